"""Emergent spectra at arbitrary wavelengths on the GPU (include/lsx_hip_spectrum.h, lsx_hip_spectrum; Engine.emergent_spectrum,
Context.compute_rays(wavelengths=...)), against the reference's own numbers (tests/golden/spectrum_falc.npz) and the checker of
tests/spectrum_cases.py: a zero-weight oracle context on the re-gridded problem.

Bars (no new numbers): against the oracle entry by entry 1e-11 |x| + 3 |x(+1) - x(-1)| from the oracle's runs with every exp(-dtau)
a ulp up / down on the re-gridded problem (tests/envelope.py); against the fixture that plus the oracle's own deviation from the
fixture, measured in the test.  A bound above 1e-8 |x| anywhere fails the test as vacuous (spectrum_cases.bound).
Every call here is an ordinary valid call or is refused on the host."""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import rays_cases as rc
import spectrum_cases as sc
from conftest import golden
from final_pass_cases import given_background, made_up_profiles, made_up_wanted
from helpers import build_data_fakes, restore_local_grids
from lightspinner_amd import _capi, fixtures, synth
from lightspinner_amd.problem import Engine
from lightspinner_amd.rh_method import Context

pytestmark = pytest.mark.gpu
FIXTURE = {'ca_vlos': 'falc_ca_vlos.npz', 'cah': 'falc_cah.npz'}
MUS6 = np.array([0.1, 0.25, 0.47, 0.6, 0.88, 1.0])


def hip_engine(hip_lib, prob, block, prof, n=None, J=None, solver='linear', **kw):
    e = Engine(prob, block.ncol, lib=hip_lib, **kw)
    synth.load_columns(e, dataclasses.replace(block, phi=None, wphi=None), prof)
    e.set_formal_solver(solver)
    if n is not None:
        e.set(_capi.LSX_N, n)
    if J is not None:
        e.set(_capi.LSX_J, J)
    return e


def inside(tag, got, runs, extra=0.0, ref=None):
    """got against the oracle (or `ref`) entry by entry inside spectrum_cases.bound; the figures are printed first"""
    x0, xp, xm = runs
    b = sc.bound(x0, xp, xm, extra)
    dev = np.abs(got - (x0 if ref is None else ref))
    print('%s: %.2e relative at worst, %.3f x the bound (envelope up to %.2e relative)'
          % (tag, float(np.max(dev / np.abs(x0))), float(np.max(dev / b)), float(np.max(np.abs(xp - xm) / np.abs(x0)))))
    assert got.shape == x0.shape and np.all(np.isfinite(got))
    assert np.all(dev <= b), tag


# ---- 1. the reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sc.CASES)
def test_engine_gives_the_reference(hip_lib, oracle_lib, case):
    prob, block, prof, n, J, mus, f = sc.fixture_case(case)
    bg = (f['bg_chi'][None], f['bg_eta'][None])
    e = hip_engine(hip_lib, prob, block, prof, n, J)
    got = e.emergent_spectrum(mus, f['w'], alpha=f['alpha'], bg_chi=bg[0], bg_eta=bg[1])
    assert got.shape == (1, f['w'].shape[0], mus.shape[0])
    runs = sc.envelope_spectrum(oracle_lib, prob, block, prof, mus, n, J, f['w'], f['alpha'], bg)
    inside('Engine %s against the oracle' % case, got, runs)
    d_ora = rc.relmax(runs[0][0], f['I'])
    print('%s: the oracle against the fixture %.2e' % (case, d_ora))
    assert d_ora <= rc.GOLDEN_BAR[case]
    inside('Engine %s against the fixture' % case, got, runs, extra=d_ora, ref=f['I'][None])
    e.close()


@pytest.mark.parametrize('case', sc.CASES)
def test_context_compute_rays_gives_the_reference(hip_lib, oracle_lib, case):
    """the drop-in Context: alpha' from the models through the library's continuum_alpha, the background as an object"""
    prob, block, prof, n, J, mus, f = sc.fixture_case(case)
    d = dict(np.load(golden(FIXTURE[case])))
    s = dict(np.load(golden('setup_falc.npz')))
    atmos, spect, eq, bgm = build_data_fakes(d, s)
    ctx = Context(atmos, spect, eq, bgm, lib=hip_lib)
    restore_local_grids(spect.radSet.activeAtoms, s)     # the continua's edges and tables: what continuum_alpha reads
    off = 0
    for atom in ctx.activeAtoms:                   # host edits of atom.n and ctx.J are sent down first
        atom.n[...] = n[0, off:off + atom.Nlevel]
        off += atom.Nlevel
    ctx.J = J[0]
    I_before, rays_before = ctx.I.copy(), ctx.compute_rays(mus)
    bgo = SimpleNamespace(chi=f['bg_chi'], eta=f['bg_eta'], sca=np.tile(block.bg_sca[0], (f['w'].shape[0], 1)))
    got = ctx.compute_rays(mus, wavelengths=f['w'], background=bgo)
    assert got.shape == (f['w'].shape[0], mus.shape[0])
    runs = sc.envelope_spectrum(oracle_lib, prob, block, prof, mus, n, J, f['w'], f['alpha'], (f['bg_chi'][None], f['bg_eta'][None]))
    d_ora = rc.relmax(runs[0][0], f['I'])
    inside('Context %s against the fixture' % case, got[None], runs, extra=d_ora, ref=f['I'][None])
    centre = ctx.compute_rays(1.0, wavelengths=f['w'], background=bgo)      # a float: no angle axis
    assert centre.shape == (f['w'].shape[0],) and np.array_equal(centre, got[:, -1])
    interp = ctx.compute_rays(mus, wavelengths=f['w'])                      # interpolation mode: an approximation, finite and close
    print('Context %s: interpolated background against the handed-over one: %.2e relative at worst' % (case, rc.relmax(interp, got)))
    assert interp.shape == got.shape and np.all(interp > 0)
    assert np.array_equal(ctx.I, I_before) and np.array_equal(ctx.compute_rays(mus), rays_before)      # today's path, bit for bit
    with pytest.raises(ValueError):
        ctx.compute_rays(mus, background=bgo)
    ctx.close()


# ---- 2. batches after MALI iterations ----------------------------------------------------------------------------------------------
def wanted(prob, nwin=120):
    """a window in the first line, points below and above the grid, a line's first and last own point and the doubles just outside,
    a point inside no transition"""
    lam = prob.wavelength
    line = next(t for t in prob.trans if t.is_line)
    lo, hi = lam[line.Nblue], lam[line.Nblue + line.Nlambda - 1]
    mid = 0.5 * (lam[1:] + lam[:-1])
    free = [x for x in mid if not any(lam[t.Nblue] <= x <= lam[t.Nblue + t.Nlambda - 1] for t in prob.trans)]
    assert free or prob.Natoms > 1, 'no wavelength outside every transition'      # (the hydrogen continua leave none)
    core = line.lambda0 + np.linspace(-0.2, 0.2, nwin)
    w = np.unique(np.concatenate([core, [0.7 * lam[0], 0.999 * lam[0], 1.5 * lam[-1], 3.0 * lam[-1]],
                                  [lo, hi, np.nextafter(lo, 0.0), np.nextafter(hi, np.inf)], free[len(free) // 2:len(free) // 2 + 1]]))
    return w


@pytest.mark.parametrize('fixture,solver', [('falc_ca.npz', 'linear'), ('falc_cah.npz', 'linear'), ('falc_ca.npz', 'parabolic')])
def test_batches_after_mali_iterations(hip_lib, oracle_lib, fixture, solver):
    ncol = 7
    prob, block, prof = rc.batch(fixture, ncol)
    e = hip_engine(hip_lib, prob, block, prof, solver=solver)
    rc.mali(e)
    n, J = e.get(_capi.LSX_N), e.get(_capi.LSX_J)
    w = wanted(prob)
    assert 125 <= w.shape[0] <= 135
    alpha = sc.interp_alpha(prob, w)
    bg = given_background(prob, block, w)
    tag = '%s %s' % (fixture, solver)
    given = e.emergent_spectrum(MUS6, w, alpha=alpha, bg_chi=bg[0], bg_eta=bg[1])
    inside(tag + ', background handed over', given, sc.envelope_spectrum(oracle_lib, prob, block, prof, MUS6, n, J, w, alpha, bg, solver))
    interp = e.emergent_spectrum(MUS6, w, alpha=alpha)
    inside(tag + ', interpolation mode', interp, sc.envelope_spectrum(oracle_lib, prob, block, prof, MUS6, n, J, w, alpha, None, solver))
    assert not np.array_equal(given, interp)
    # a column's result does not depend on the call: a sub-range, passes of one column, passes of three, the column alone in an engine
    assert np.array_equal(e.emergent_spectrum(MUS6, w, alpha=alpha, col0=2, ncol=3), interp[2:5])
    assert np.array_equal(e.emergent_spectrum(MUS6, w, alpha=alpha, bg_chi=bg[0][2:5], bg_eta=bg[1][2:5], col0=2, ncol=3), given[2:5])
    per_col = (w.shape[0] * MUS6.shape[0] + 4 * w.shape[0] * prob.Nspace) * 8
    assert np.array_equal(e.emergent_spectrum(MUS6, w, alpha=alpha, bg_chi=bg[0], bg_eta=bg[1], work_cap_bytes=1), given)
    assert np.array_equal(e.emergent_spectrum(MUS6, w, alpha=alpha, bg_chi=bg[0], bg_eta=bg[1], work_cap_bytes=3 * per_col + 64), given)
    assert np.array_equal(e.emergent_spectrum(MUS6, w, alpha=alpha, work_cap_bytes=2 * w.shape[0] * MUS6.shape[0] * 8), interp)
    assert np.array_equal(e.emergent_spectrum(MUS6, w, alpha=alpha, bg_chi=bg[0], bg_eta=bg[1], work_cap_bytes=0), given)
    e.close()
    for c in (0, 3, 6):
        one = hip_engine(hip_lib, prob, block.slice(c, c + 1), tuple(x[c:c + 1] for x in prof), n[c:c + 1], J[c:c + 1], solver=solver)
        assert np.array_equal(one.emergent_spectrum(MUS6, w, alpha=alpha), interp[c:c + 1]), c
        assert np.array_equal(one.emergent_spectrum(MUS6, w, alpha=alpha, bg_chi=bg[0][c:c + 1], bg_eta=bg[1][c:c + 1]), given[c:c + 1]), c
        one.close()


# ---- 3. any subset of the wavelengths or angles is the rows of the full call ----------------------------------------------------
def test_subsets_of_wavelengths_and_angles(hip_lib):
    prob, block, prof, n, J, _, _ = rc.golden_case('ca_vlos')
    e = hip_engine(hip_lib, prob, block, prof, n, J)
    w = wanted(prob, nwin=121)
    assert w.shape[0] == 130
    alpha = sc.interp_alpha(prob, w)
    bg = given_background(prob, block, w)
    mus = np.linspace(0.1, 1.0, 15)
    full = {False: e.emergent_spectrum(mus, w, alpha=alpha), True: e.emergent_spectrum(mus, w, alpha=alpha, bg_chi=bg[0], bg_eta=bg[1])}
    rng = np.random.default_rng(5)
    for nla in (1, 63, 64, 65, 130):
        for nmu in (1, 3, 7, 15):
            qs = np.sort(rng.choice(130, nla, replace=False))
            ms = np.sort(rng.choice(15, nmu, replace=False))
            for given in (False, True):
                kw = dict(bg_chi=bg[0][:, qs], bg_eta=bg[1][:, qs]) if given else {}
                part = e.emergent_spectrum(mus[ms], w[qs], alpha=alpha[:, qs], **kw)
                assert np.array_equal(part, full[given][:, qs][:, :, ms]), (nla, nmu, given)
    e.close()


# ---- 4. on the context's own grid --------------------------------------------------------------------------------------------------
def test_on_the_own_grid(hip_lib, oracle_lib):
    prob, block, prof = rc.batch('falc_ca.npz', 3)
    e = hip_engine(hip_lib, prob, block, prof)
    rc.mali(e)
    n, J = e.get(_capi.LSX_N), e.get(_capi.LSX_J)
    w = prob.wavelength
    alpha = np.zeros((prob.Ntrans - prob.Nlines, prob.Nspect))
    for kc, t in enumerate(t for t in prob.trans if not t.is_line):
        alpha[kc, t.Nblue:t.Nblue + t.Nlambda] = t.alpha
    rays = e.emergent_rays(MUS6)
    given = e.emergent_spectrum(MUS6, w, alpha=alpha, bg_chi=block.bg_chi, bg_eta=block.bg_eta)
    interp = e.emergent_spectrum(MUS6, w, alpha=alpha)
    runs = rc.envelope_runs(oracle_lib, prob, block, prof, MUS6, n, J)
    runs = tuple(runs[u][0][_capi.LSX_I] for u in (0, 1, -1))
    inside('own grid, lsx_hip_emergent_rays', rays, runs)
    inside('own grid, background handed over', given, runs)
    inside('own grid, interpolation mode', interp, runs)
    assert np.all(np.abs(given - rays) <= sc.bound(*runs)) and np.all(np.abs(interp - rays) <= sc.bound(*runs))
    print('own grid: against lsx_hip_emergent_rays %s (%.1e relative at worst); interpolation mode against the handed-over background %s'
          % ('bit-equal' if np.array_equal(given, rays) else 'not bit-equal', rc.relmax(given, rays),
             'bit-equal' if np.array_equal(given, interp) else 'not bit-equal'))
    e.close()


# ---- 5. depth limits, scattering per wavelength --------------------------------------------------------------------------------------
@pytest.mark.parametrize('solver', ['linear', 'parabolic'])
def test_three_depths(hip_lib, oracle_lib, solver):
    """the smallest atmosphere lsx_create admits: the boundary value, one ordinary step (none under the parabolic rule) and the end point"""
    import instance_cases as ic
    prob, block = ic.build('two_atoms', 3, 3, False)
    prof = made_up_profiles(prob, block)
    e = hip_engine(hip_lib, prob, block, prof, solver=solver)
    e.formal_sol_gamma()
    e.formal_sol_gamma()
    n, J = e.get(_capi.LSX_N), e.get(_capi.LSX_J)
    w = made_up_wanted(prob)
    alpha, bg = sc.interp_alpha(prob, w), given_background(prob, block, w)
    mus = np.array([0.2, 0.7, 1.0])
    got = e.emergent_spectrum(mus, w, alpha=alpha, bg_chi=bg[0], bg_eta=bg[1])
    inside('three depths %s' % solver, got, sc.envelope_spectrum(oracle_lib, prob, block, prof, mus, n, J, w, alpha, bg, solver))
    e.close()


def test_scattering_per_wavelength(hip_lib, oracle_lib):
    from toy import toy_problem
    prob, block = toy_problem(seed=3, Nspace=37, Nrays=3, Nspect=90, ncol=3, sca_per_lambda=True)
    prof = made_up_profiles(prob, block)
    e = hip_engine(hip_lib, prob, block, prof)
    e.formal_sol_gamma()
    e.formal_sol_gamma()
    n, J = e.get(_capi.LSX_N), e.get(_capi.LSX_J)
    w = made_up_wanted(prob)
    alpha, bg = sc.interp_alpha(prob, w), given_background(prob, block, w)
    mus = np.array([0.2, 0.7, 1.0])
    got = e.emergent_spectrum(mus, w, alpha=alpha, bg_chi=bg[0], bg_eta=bg[1], bg_sca=bg[2])
    inside('sca_per_lambda, handed over', got, sc.envelope_spectrum(oracle_lib, prob, block, prof, mus, n, J, w, alpha, bg))
    got = e.emergent_spectrum(mus, w, alpha=alpha)
    inside('sca_per_lambda, interpolation mode', got, sc.envelope_spectrum(oracle_lib, prob, block, prof, mus, n, J, w, alpha, None))
    f = hip_lib.dll.lsx_hip_spectrum
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    out = np.zeros((3, w.shape[0], 3))
    args = lambda sca: (e._h, w.shape[0], dp(w), dp(alpha), dp(bg[0]), dp(bg[1]), sca, 3, dp(mus), 0, 3, dp(out), out.nbytes)
    assert f(*args(None)) == _capi.LSX_EINVAL and not out.any()          # bg_sca is missing
    e.close()


def test_325_depths(hip_lib, oracle_lib):
    from parabolic_cases import _refine_depth
    prob, base, raw = fixtures.load_problem_npz(golden('falc_ca.npz'))
    coarse, _ = synth.perturbed_columns(prob, base, raw, ncol=3, seed=4242, vlos_sigma=0.0)
    fine, fblock, xf = _refine_depth(prob, coarse, 4)
    assert fine.Nspace == 325
    aD, vB, _ = fixtures.profile_inputs(prob, raw, with_vlos=False)
    x = np.arange(prob.Nspace, dtype=np.float64)
    up = lambda a: np.stack([np.interp(xf, x, r) for r in a.reshape(-1, prob.Nspace)]).reshape(a.shape[:-1] + (325,))
    prof = (np.repeat(up(aD), 3, axis=0), np.repeat(up(vB), 3, axis=0), None)
    fine = dataclasses.replace(fine, phi_compact=False)
    e = hip_engine(hip_lib, fine, fblock, prof)
    rc.mali(e)
    n, J = e.get(_capi.LSX_N), e.get(_capi.LSX_J)
    w = wanted(fine, nwin=40)
    alpha = sc.interp_alpha(fine, w)
    mus = np.array([0.15, 0.5, 1.0])
    got = e.emergent_spectrum(mus, w, alpha=alpha)
    inside('325 depths', got, sc.envelope_spectrum(oracle_lib, fine, fblock, prof, mus, n, J, w, alpha, None))
    e.close()


# ---- 6. read-only ---------------------------------------------------------------------------------------------------------------
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
    w = wanted(prob, nwin=60)
    alpha, bg = sc.interp_alpha(prob, w), given_background(prob, block, w)
    engines = [hip_engine(hip_lib, prob, block, prof) for _ in range(2)]
    probe, twin = engines
    seen = []
    for it in range(4):
        for e in engines:
            e.formal_sol_gamma()
        seen.append(probe.emergent_spectrum(mus, w, alpha=alpha))
        assert same_state(snapshot(probe), snapshot(twin))
        if it >= 2:
            for e in engines:
                e.stat_equil()
            seen.append(probe.emergent_spectrum(mus, w, alpha=alpha, bg_chi=bg[0][1:-1], bg_eta=bg[1][1:-1], col0=1, ncol=ncol - 2))
            assert same_state(snapshot(probe), snapshot(twin))
    # the pipelined loop: FS; SE; sync_begin; speculative FS; [the call]; sync_end; discard
    for e in engines:
        e.formal_sol_gamma_async()
        e.stat_equil_async()
        e.sync_begin()
        e.formal_sol_gamma_speculative()
    spec = probe.emergent_spectrum(mus, w, alpha=alpha)            # sees what lsx_get sees: the speculative call's J
    assert np.array_equal(probe.get(_capi.LSX_J), twin.get(_capi.LSX_J))
    mon = [e.sync_end() for e in engines]
    assert mon[0] == mon[1]
    assert same_state(snapshot(probe), snapshot(twin))
    for e in engines:
        e.discard_formal_sol()
    assert same_state(snapshot(probe), snapshot(twin))
    back = probe.emergent_spectrum(mus, w, alpha=alpha)            # the accepted call's J again
    assert not np.array_equal(back, spec)
    for e in engines:                                              # and the following calls produce the bits they would have produced
        e.formal_sol_gamma()
        e.stat_equil()
        e.formal_sol_gamma()
    assert same_state(snapshot(probe), snapshot(twin))
    assert all(np.all(np.isfinite(x)) and np.all(x > 0) for x in seen + [spec, back])
    # frozen columns are computed like any other
    d = probe.emergent_spectrum(mus, w, alpha=alpha)
    probe.set_active_columns(np.arange(ncol) % 3 != 0)
    assert np.array_equal(probe.emergent_spectrum(mus, w, alpha=alpha), d)
    for e in engines:
        e.close()


# ---- 7. errors are found on the host ---------------------------------------------------------------------------------------------
def test_errors(hip_lib):
    prob, block, prof = rc.batch('falc_ca.npz', 4)
    e = Engine(prob, 4, lib=hip_lib)
    e.set_columns(0, block)                       # profiles not set yet
    w = np.array([392.0, 393.4, 854.2, 854.25, 2000.0])
    alpha = sc.interp_alpha(prob, w)
    with pytest.raises(_capi.LsxError) as err:
        e.emergent_spectrum([1.0], w, alpha=alpha)
    assert err.value.code == _capi.LSX_EINVAL and 'no line profiles' in str(err.value)
    e.set_line_profiles(0, *prof)
    e.formal_sol_gamma()
    before, rays_before = snapshot(e), e.emergent_rays([0.5, 1.0])
    f = hip_lib.dll.lsx_hip_spectrum
    NLA = w.shape[0]
    out = np.zeros((4, NLA, 2))
    bg = given_background(prob, block, w)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))      # (float64, contiguous, kept alive by the caller)

    def call(mus=(0.5, 1.0), wl=w, al=alpha, chi=None, eta=None, sca=None, col0=0, ncol=4, nbytes=None, nmu=None, nla=None):
        mu = np.asarray(mus, dtype=np.float64)
        wl = np.asarray(wl, dtype=np.float64)
        return f(e._h, len(wl) if nla is None else nla, dp(wl), dp(al), dp(chi), dp(eta), dp(sca), len(mu) if nmu is None else nmu, dp(mu),
                 col0, ncol, out.ctypes.data_as(C.POINTER(C.c_double)), out.nbytes if nbytes is None else nbytes)
    assert call() == 0
    assert call(chi=bg[0], eta=bg[1]) == 0
    good = out.copy()
    for bad in ([0.5, 0.0], [0.5, -0.2], [1.0000001, 0.5], [0.5, np.nan], [np.inf, 0.5]):
        assert call(mus=bad) == _capi.LSX_EINVAL, bad
    assert call(nmu=0) == _capi.LSX_EINVAL and call(nmu=-1) == _capi.LSX_EINVAL
    assert call(nla=0) == _capi.LSX_EINVAL and call(nla=-2) == _capi.LSX_EINVAL
    for bad in ([393.4, 392.0, 854.2, 854.25, 2000.0], [392.0, 393.4, 393.4, 854.25, 2000.0], [392.0, 393.4, np.nan, 854.25, 2000.0],
                [392.0, 393.4, 854.2, 854.25, np.inf], [0.0, 393.4, 854.2, 854.25, 2000.0], [-5.0, 393.4, 854.2, 854.25, 2000.0]):
        assert call(wl=bad) == _capi.LSX_EINVAL, bad
    assert call(col0=-1) == _capi.LSX_EINVAL and call(col0=1, ncol=4) == _capi.LSX_EINVAL and call(ncol=0) == _capi.LSX_EINVAL
    assert call(ncol=3) == _capi.LSX_EINVAL                           # the byte count is that of four columns
    assert call(nbytes=out.nbytes - 8) == _capi.LSX_EINVAL and call(nla=NLA - 1) == _capi.LSX_EINVAL
    assert call(chi=bg[0]) == _capi.LSX_EINVAL and call(eta=bg[1]) == _capi.LSX_EINVAL
    assert call(chi=bg[0], eta=bg[1], sca=bg[0]) == _capi.LSX_EINVAL     # not a sca_per_lambda context
    assert call(sca=bg[0]) == _capi.LSX_EINVAL
    assert call(al=None) == _capi.LSX_EINVAL
    assert np.array_equal(out, good) and same_state(snapshot(e), before)      # nothing launched or written
    assert np.array_equal(e.emergent_rays([0.5, 1.0]), rays_before)
    e.close()
    # profiles handed over as arrays: the library cannot know them at another wavelength -- ray dependent or compact
    for compact in (False, True):
        prob, base, raw = fixtures.load_problem_npz(golden('falc_ca.npz'), phi_compact=compact)
        e = Engine(prob, 1, lib=hip_lib)
        e.set_columns(0, base)
        with pytest.raises(_capi.LsxError) as err:
            e.emergent_spectrum([1.0], w, alpha=alpha)
        assert err.value.code == _capi.LSX_EUNSUPPORTED
        assert 'lsx_set_line_profiles' in str(err.value) and 'lsx_set_atmosphere' in str(err.value)
        assert np.all(e.get(_capi.LSX_N) > 0)                          # nothing was launched: a following lsx_get works
        e.set_line_profiles(0, *fixtures.profile_inputs(prob, raw, with_vlos=False))     # ... and can once it has built them itself
        assert np.all(e.emergent_spectrum([0.2, 1.0], w, alpha=alpha) > 0)
        e.close()
