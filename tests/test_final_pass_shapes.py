"""The four read-only final-pass entries on the GPU, off the FALC shape: lsx_hip_radiative_rates, lsx_hip_emergent_rays,
lsx_hip_depth_rays and lsx_hip_spectrum on the made-up problems of tests/final_pass_cases.py -- 1 to 64 rays (every group of rays
lsx_rates.hip launches, as the first group of a call and as a later one; tile widths of 64 down to 1 wavelength), the toy
topologies, a problem without continua, columns of 3 to 45 depths.

No new bars: the rates inside rates_cases.BASE |x| + 3 |x(+1) - x(-1)| of rates_cases.oracle_runs, the emergent intensities inside
1e-11 |x| + 3 |x(+1) - x(-1)| of rays_cases.envelope_runs, the depth-resolved arrays by tests/test_depth_rays.py's check_column,
the spectra through tests/test_spectrum.py's inside -- entry by entry, which tests/test_final_pass_shapes_host.py shows to be
meaningful on every case (all entries positive, no bound above 1e-9 relative).  Every test prints its worst deviation and its
ratio to the bound.  Every call here is an ordinary valid call.

Measured on the MI355X, worst over all cases and both rules ("The final pass off the FALC shape"): rates 4.5e-15
relative, < 0.001 x the bound; emergent rays 4.0e-13, 0.032 x; quadrature angles against LSX_I 5.5e-13, 0.041 x; depth rays I(k)
4.1e-13, 0.032 x; spectrum 9.7e-14, 0.009 x.

Last, the seven entries whose passes run under a cap (these four without the emergent rays, the Stokes pass, its response and the
field fit) one after the other on one context, bit for bit against fresh contexts."""
import numpy as np
import pytest

import depth_cases as dc
import envelope
import final_pass_cases as fp
import rates_cases as rt
import rays_cases as rc
import spectrum_cases as sc
import test_depth_rays as tdr
import test_radiative_rates as trr
import test_spectrum as tsp
from lightspinner_amd import _capi

pytestmark = pytest.mark.gpu
LSX_I, LSX_J, LSX_N = _capi.LSX_I, _capi.LSX_J, _capi.LSX_N
SUBSETS = {20: slice(None), 7: slice(0, 20, 3), 5: slice(1, 20, 4), 1: slice(19, 20)}     # angles of MUS20: chunks of 8, 4, 2 and 1
DEPTH_MUS = np.array([0.1, 0.33, 0.6, 0.85, 1.0])                                         # register chunks of 4 + 1
SPECTRUM_MUS = rc.MUS20[::4]


def engine_in_state(hip_lib, name, solver, blk, prof):
    """-> (engine, n, J): the HIP engine of a case in the state the case is evaluated in"""
    prob, _ = fp.build(name)
    e = trr.hip_engine(hip_lib, prob, blk, prof, solver=solver)
    fp.reach_state(e, fp.BY_NAME[name])
    return e, e.get(LSX_N), e.get(LSX_J)


# ---- radiative rates: every case under both rules ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name,solver', fp.RATES_PARAMS)
def test_rates_meet_the_oracle(hip_lib, oracle_lib, name, solver):
    """the toy block's own profile arrays, ray and direction dependent where the case is not compact: the profile index of a later
    group is ((dir Ns + k) Nrays + mu0 + m)"""
    prob, block = fp.build(name)
    e, n, J = engine_in_state(hip_lib, name, solver, block, None)
    before = trr.snapshot(e)
    r = e.radiative_rates()
    assert r.Rij.shape == r.Rji.shape == r.Rji_ref.shape == (block.ncol, prob.Ntrans, prob.Nspace)
    tag = '%s %s (groups of %s rays)' % (name, solver, ' + '.join(str(g) for g in fp.BY_NAME[name].groups))
    trr.inside_oracle(tag, r, rt.oracle_runs(oracle_lib, prob, block, None, n, J, solver))
    assert trr.same_rates(e.radiative_rates(), r)                                      # nothing is accumulated over calls
    if name == fp.SEVEN_COLUMNS:
        assert block.ncol == 7 and len(fp.BY_NAME[name].groups) > 1
        assert trr.same_rates(e.radiative_rates(col0=2, ncol=3), r, slice(2, 5))       # a column sub-range
        per_col = 8 * prob.Nspace * (prob.Nspect + 2 * prob.SNl)
        assert trr.same_rates(e.radiative_rates(work_cap_bytes=2 * per_col + 64), r)   # passes of 2 + 2 + 2 + 1 columns
        assert trr.same_rates(e.radiative_rates(work_cap_bytes=1), r)                  # below one column's need: one column per pass
        assert trr.same_rates(e.radiative_rates(col0=1, ncol=5, work_cap_bytes=2 * per_col + 64), r, slice(1, 6))
        assert trr.same_rates(e.radiative_rates(work_cap_bytes=0), r)
    assert trr.same(trr.snapshot(e), before)                                           # I, J, Gamma, n and the monitors: untouched
    e.close()


@pytest.mark.parametrize('solver', fp.SOLVERS)
def test_a_frozen_column_at_eight_rays_is_computed_like_any_other(hip_lib, solver):
    prob, block = fp.build(fp.FROZEN)
    assert prob.Nrays == 8
    e, n, J = engine_in_state(hip_lib, fp.FROZEN, solver, block, None)
    r = e.radiative_rates()
    mask = np.array([True, False, True])
    e.set_active_columns(mask)
    assert trr.same_rates(e.radiative_rates(), r)
    e.formal_sol_gamma()                          # the frozen column keeps its J: its rates stay, the others move
    r2 = e.radiative_rates()
    assert np.array_equal(r2.Rij[~mask], r.Rij[~mask]) and not np.array_equal(r2.Rij[mask], r.Rij[mask])
    assert np.array_equal(r2.Rji[~mask], r.Rji[~mask]) and np.array_equal(r2.Rji_ref[~mask], r.Rji_ref[~mask])
    e.close()


# ---- emergent rays -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,solver', fp.RATES_PARAMS)
def test_emergent_rays_meet_the_oracle(hip_lib, oracle_lib, name, solver):
    prob, block = fp.build(name)
    blk, prof = fp.rays_inputs(prob, block)
    e, n, J = engine_in_state(hip_lib, name, solver, blk, prof)
    runs = rc.envelope_runs(oracle_lib, prob, blk, prof, rc.MUS20, n, J, solver)
    full = None
    for nmu, sel in SUBSETS.items():
        mus = rc.MUS20[sel]
        assert mus.shape[0] == nmu
        I = e.emergent_rays(mus)
        sub = rc.runs_subset(runs, angles=sel)
        assert I.shape == (block.ncol, prob.Nspect, nmu) and np.all(np.isfinite(I))
        ratio, rel, renv = envelope.excess(I, sub, 0, LSX_I, 1e-11)
        print('%s %s L=%d nmu=%d: largest deviation %.2e relative, largest envelope %.2e relative, %.3f x the bound'
              % (name, solver, 64 // prob.Nrays, nmu, rel, renv, ratio))
        envelope.inside(I, sub, 0, LSX_I, base=1e-11)
        if nmu == 20:
            full = I
    assert np.array_equal(e.emergent_rays(rc.MUS20, col0=1, ncol=block.ncol - 1), full[1:])
    e.close()


@pytest.mark.parametrize('name,solver', [(name, s) for name in fp.QUADRATURE for s in fp.SOLVERS])
def test_quadrature_angles_reproduce_the_formal_solution(hip_lib, oracle_lib, name, solver):
    """1, 7, 8 and 64 rays: the sweep kernels and the final pass are one formal solution of identical inputs"""
    prob, block = fp.build(name)
    blk, prof = fp.rays_inputs(prob, block)
    e, n, Jd = engine_in_state(hip_lib, name, solver, blk, prof)
    e.formal_sol_gamma()
    I_fs = e.get(LSX_I)
    e.set(LSX_J, Jd)
    I = e.emergent_rays(prob.muz)
    runs = rc.envelope_runs(oracle_lib, prob, blk, prof, prob.muz, n, Jd, solver)
    for tag, x in (('lsx_hip_emergent_rays', I), ('LSX_I of the formal solution', I_fs)):
        ratio, rel, renv = envelope.excess(x, runs, 0, LSX_I, 1e-11)
        print('%s %s, %d quadrature angles, %s: largest deviation %.2e relative, largest envelope %.2e relative, %.3f x the bound'
              % (name, solver, prob.Nrays, tag, rel, renv, ratio))
    envelope.inside(I, runs, 0, LSX_I, base=1e-11)
    envelope.inside(I_fs, runs, 0, LSX_I, base=1e-11)
    x0, env = runs[0][0][LSX_I], envelope.envelope(runs, 0, LSX_I)
    assert np.all(np.abs(I - I_fs) <= 1e-11 * np.abs(x0) + envelope.K_ENVELOPE * env)
    e.close()


# ---- depth rays --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,solver', [(name, s) for name, rules in fp.DEPTH for s in rules])
def test_depth_rays_meet_every_bar(hip_lib, oracle_lib, name, solver):
    prob, block = fp.build(name)
    blk, prof = fp.rays_inputs(prob, block)
    e, n, J = engine_in_state(hip_lib, name, solver, blk, prof)
    mus = DEPTH_MUS
    d = e.depth_rays(mus)
    assert d.I.shape == (block.ncol, mus.shape[0], prob.Nspace, prob.Nspect)
    phi = block.phi if prob.phi_compact else dc.profiles_at(hip_lib, prob, blk, prof, mus)
    tag = '%s %s' % (name, solver)
    runs = [tdr.check_column('%s column %d' % (tag, c), oracle_lib, prob, blk, c, n[c], J[c], phi[c], d, c, solver=solver)[2]
            for c in range(block.ncol)]
    tdr.top_against_emergent_rays(tag, e, d, runs, check=True)
    # I[..., 0] against the reference's final pass as the oracle's zero-weight context restates it, inside its envelope
    zw = rc.envelope_runs(oracle_lib, prob, blk, prof, mus, n, J, solver)
    top = np.stack([dc.to_lambda_major(d.I[c])[:, :, 0] for c in range(block.ncol)])
    ratio, rel, renv = envelope.excess(top, zw, 0, LSX_I, 1e-11)
    print('%s: I[..., 0] against the zero-weight oracle context: %.2e relative (envelope up to %.2e), %.3f x the bound' % (tag, rel, renv, ratio))
    envelope.inside(top, zw, 0, LSX_I, base=1e-11)
    assert dc.same(e.depth_rays(mus, col0=1, ncol=2), d, slice(1, 3))
    # a window that starts inside a tile and ends inside another is a slice of the full call
    la0, nla = prob.Nspect // 3 + 1, prob.Nspect // 2
    w = e.depth_rays(mus, la0=la0, nla=nla)
    assert all(np.array_equal(getattr(w, f), getattr(d, f)[..., la0:la0 + nla], equal_nan=True) for f in tdr.FIELDS)
    e.close()


# ---- spectrum ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,solver', [(name, s) for name, rules in fp.SPECTRUM for s in rules])
def test_spectrum_meets_the_oracle(hip_lib, oracle_lib, name, solver):
    prob, block = fp.build(name)
    blk, prof = fp.library_profiles(prob, block)
    assert (prof[2] is None) == prob.phi_compact
    e, n, J = engine_in_state(hip_lib, name, solver, blk, prof)
    w = fp.made_up_wanted(prob)
    alpha, bg = sc.interp_alpha(prob, w), fp.given_background(prob, block, w)
    assert (alpha is None) == (name == 'lines-only')
    mus = SPECTRUM_MUS
    kw = dict(bg_chi=bg[0], bg_eta=bg[1])
    if prob.sca_per_lambda:
        kw['bg_sca'] = bg[2]
    tag = '%s %s L=%d' % (name, solver, 64 // prob.Nrays)
    given = e.emergent_spectrum(mus, w, alpha=alpha, **kw)
    assert given.shape == (block.ncol, w.shape[0], mus.shape[0])
    tsp.inside(tag + ', background handed over', given, sc.envelope_spectrum(oracle_lib, prob, blk, prof, mus, n, J, w, alpha, bg, solver))
    interp = e.emergent_spectrum(mus, w, alpha=alpha)
    tsp.inside(tag + ', interpolation mode', interp, sc.envelope_spectrum(oracle_lib, prob, blk, prof, mus, n, J, w, alpha, None, solver))
    assert not np.array_equal(given, interp)
    assert np.array_equal(e.emergent_spectrum(mus, w, alpha=alpha, col0=1, ncol=2), interp[1:3])
    e.close()


# ---- the seven capped passes on one context ------------------------------------------------------------------------------------------
def test_the_capped_passes_keep_their_own_buffers_on_one_context(hip_lib):
    """Rates, losses, depth rays, spectrum, Stokes rays, their response and the field fit keep their passes under a cap each, in a
    buffer each (lsx_ctx.h, GrowBuf).  On ONE context, one after the other: first every cap at one column's need -- three passes an
    entry, every work buffer freed and allocated anew -- then every cap back at its default.  Every result is, bit for bit, that of
    the same call on a fresh context that has seen no other call: no two passes on the same storage (the fit holds its buffer while
    the Stokes pass and the response run inside it, the response entry runs the Stokes pass behind its own), every cap at its own
    buffer."""
    import fit_cases as fc
    import stokes_cases as stc
    import stokes_response_cases as src
    from lightspinner_amd.problem import Engine, RadiativeLosses
    from lightspinner_amd import synth
    Ns, ncol, nnode = 3, 3, (2, 2, 2)
    prob, block, prof, J = stc.problem(Ns, ncol, vlos=True)
    fld, pats, mus = stc.field(Ns, ncol), stc.PATTERN_SETS['all'], fc.MUS
    nmu, nla, P = mus.shape[0], prob.Nspect, sum(nnode)
    w = fp.made_up_wanted(prob)
    alpha, bg = sc.interp_alpha(prob, w), fp.given_background(prob, block, w)
    bgkw = dict(bg_chi=bg[0], bg_eta=bg[1], **({'bg_sca': bg[2]} if prob.sca_per_lambda else {}))
    basis, nodes = fc.basis_of(Ns, nnode), fc.nodes_of(fld, Ns, nnode)

    def fresh():
        e = Engine(prob, ncol, lib=hip_lib)
        synth.load_columns(e, block, prof)
        e.set(LSX_J, J)
        return e

    def stokes(e, **kw):
        r = e.stokes_rays(mus, *fld, patterns=pats, **kw)
        return [r.I, r.Q, r.U, r.V]

    e0 = fresh()
    obs = np.stack(stokes(e0), axis=1) * 1.01
    e0.close()

    def response(e, **kw):
        r = e.stokes_response(mus, *fld, patterns=pats, amplitudes=src.AMPS, **kw)
        return [src.stack_rf(r), r.stokes.I, r.stokes.Q, r.stokes.U, r.stokes.V]

    def fit(e, **kw):
        ne = e.fit_field_normal(mus, basis, nnode, nodes, obs, patterns=pats, amplitudes=fc.AMPS, **kw)
        step = e.fit_field_step(ne.hess, ne.grad, 1.0, nodes)               # (the step lays its own arrays out in the fit's buffer)
        c2 = e.fit_field_chi2(mus, basis, nnode, nodes, obs, patterns=pats)[0]
        return [ne.chi2, ne.grad, ne.hess, ne.field, c2, *step]

    # one column's need of every pass in bytes, as the units count it (their "columns per pass" paragraphs)
    nlaP, nw, M = 64 * ((nla + 63) // 64), w.shape[0], 4 * nla * nmu
    nstream = 3 if prob.sca_per_lambda else 2
    passes = [
        ('rates', lambda e, **kw: [getattr(e.radiative_rates(**kw), f) for f in ('Rij', 'Rji', 'Rji_ref')], Ns * (prob.Nspect + 2 * prob.SNl)),
        ('losses', lambda e, **kw: [getattr(e.radiative_losses(what=RadiativeLosses.FIELDS, **kw), f) for f in RadiativeLosses.FIELDS],
         Ns * (3 * prob.Nspect + 2 * prob.SNl)),
        ('depth', lambda e, **kw: [getattr(e.depth_rays(mus, **kw), f) for f in tdr.FIELDS], 5 * nmu * nla * Ns + nmu * nla),
        ('spectrum', lambda e, **kw: [e.emergent_spectrum(mus, w, alpha=alpha, **bgkw, **kw)], nw * nmu + 2 * nstream * nw * Ns),
        ('stokes', stokes, M + 3 * Ns),
        ('response', response, nmu * 7 * Ns * 11 * nlaP + nmu * Ns * 5 * nlaP + 3 * M * Ns + 3 * Ns),
        ('fit', fit, 2 * M + 2 * M + P * M + 1 + P + P * P),
    ]
    want = {}
    for name, run, _ in passes:
        e0 = fresh()
        want[name] = run(e0)
        finite = want[name][:-1] if name == 'depth' else want[name]           # (a height of tau = 1 need not exist)
        assert all(np.all(np.isfinite(a)) for a in finite), name
        e0.close()
    e = fresh()
    for rnd, cap_of in (('one column a pass', lambda doubles: 8 * doubles), ('default caps', lambda doubles: 0)):
        for name, run, doubles in passes:
            got = run(e, work_cap_bytes=cap_of(doubles))
            assert len(got) == len(want[name])
            for i, (a, b) in enumerate(zip(got, want[name])):
                assert np.array_equal(a, b, equal_nan=True), (rnd, name, i)
    e.close()
