"""Radiative flux, net cooling and its division among the transitions on the GPU (include/lsx_hip_losses.h,
lsx_hip_radiative_losses; Engine.radiative_losses, Context.compute_losses) against the unmodified reference's own formal solution
(tests/golden/losses_falc_*.npz, tests/golden/make_losses_golden.py) and against identities on made-up problems.

Every comparison is relative to the GROSS of the quantity (all terms positive), never to its value: deep down eta - chi I cancels
to nothing.  The bar is tests/losses_cases.py's, computed and not typed: BASE gross + K_ENVELOPE x (the quantity's own linear
dependence on the intensity, every coefficient positive, applied to |J(+1) - J(-1)| of the oracle's one-ulp-exponential runs).
Every test prints its largest deviation and its ratio to the bound.  Every call here is an ordinary valid call or is refused on
the host.

Measured on the MI355X ("Radiative flux and net cooling"), largest ratio to the bound: fixture states H 0.019, D 0.041
(Ca + H after se5), Qt 0.013, F and Q below 0.0005; the identities on the made-up problems and at 325 depths below 0.0005 (deviations
of 2e-16 ... 8e-15 of the gross); a line's Qt against (hc / lambda_0) net() on the five-atom problem 0.005."""
import ctypes as C

import numpy as np
import pytest

import final_pass_cases as fp
import losses_cases as lc
import rates_cases as rt
import rays_cases as rc
from conftest import golden
from helpers import build_fakes
from lightspinner_amd import _capi, fixtures, synth
from lightspinner_amd import constants as Const
from lightspinner_amd.problem import Engine, RadiativeLosses
from lightspinner_amd.rh_method import Context

pytestmark = pytest.mark.gpu
ALL = RadiativeLosses.FIELDS
LSX_I, LSX_J, LSX_N = _capi.LSX_I, _capi.LSX_J, _capi.LSX_N


def hip_engine(hip_lib, prob, block, prof, n=None, J=None, solver='linear', **kw):
    e = Engine(prob, block.ncol, lib=hip_lib, **kw)
    synth.load_columns(e, block, prof)
    e.set_formal_solver(solver)
    if n is not None:
        e.set(LSX_N, n)
    if J is not None:
        e.set(LSX_J, J)
    return e


def same_losses(a, b, cols=slice(None), fields=ALL):
    return all(np.array_equal(getattr(a, f), getattr(b, f)[cols]) for f in fields)


def snapshot(e):
    return {w: e.get(w) for w in (LSX_I, LSX_J, _capi.LSX_GAMMA, LSX_N, _capi.LSX_DJ_COL, _capi.LSX_DPOPS_COL)}


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


# ---- 1. the three fixture states, under both store layouts of the profiles ----------------------------------------------------------
FIXTURE_PARAMS = [('ca', 'compact'), ('ca', 'per-ray'), ('cah', 'compact'), ('cah', 'per-ray'), ('ca_vlos', 'built'), ('ca_vlos', 'arrays')]


def flux_divergence_report(prob, block, L):
    """reported, not gated: dF/dz by centred differences against Q, per depth band (a discretisation statement: DESIGN.md 4.19)"""
    z, F, Q = block.height[0], L.F[0], L.Q[0]
    dFdz = (F[:-2] - F[2:]) / (z[:-2] - z[2:])
    rel = np.abs(dFdz - Q[1:-1]) / np.maximum(np.abs(Q[1:-1]), 1e-300)
    for lo in range(0, rel.shape[0], 16):
        sl = slice(lo, min(lo + 16, rel.shape[0]))
        print('  depths %2d-%2d: |dF/dz - Q| / |Q| median %.2e, largest %.2e; Q from %.3e to %.3e W m-3'
              % (lo + 1, sl.stop, float(np.median(rel[sl])), float(np.max(rel[sl])), Q[1:-1][sl].min(), Q[1:-1][sl].max()))


@pytest.mark.parametrize('case,layout', FIXTURE_PARAMS)
def test_the_fixture_states_meet_the_reference(hip_lib, oracle_lib, case, layout):
    prob, block, prof, n, J = lc.state(case, phi_compact=False if layout == 'per-ray' else None)
    assert prob.phi_compact == (layout == 'compact')
    e = hip_engine(hip_lib, prob, block, prof, n, J)
    if layout == 'arrays':                         # the 4-D profiles handed over through lsx_set_columns: no kept profile inputs
        block2 = rt.with_profile_arrays(e, block)
        built = e.radiative_losses(what=ALL)
        e.close()
        e = hip_engine(hip_lib, prob, block2, None, n, J)
    L = e.radiative_losses(what=ALL)
    if layout == 'arrays':                         # the same numbers in the store, whoever put them there
        assert same_losses(L, built)
    phi, wphi = e.get(_capi.LSX_PHI)[0], e.get(_capi.LSX_WPHI)[0]
    e.close()
    fx = lc.fixture(case)
    idx = fx['la_idx']
    assert np.array_equal(L.wnu, fx['wnu'])
    dJ, _ = lc.pass_envelope(oracle_lib, prob, block, prof, n, J)
    dJ = dJ[0]
    chi = lc.chi_max(prob, block, n[0], phi)
    wabs = np.abs(L.wnu)
    tag = '%s %s' % (case, layout)
    r = [lc.ratio(tag, 'H', L.H[0][idx], fx['H'], fx['Hg'], dJ[idx]),
         lc.ratio(tag, 'D', L.D[0][idx], fx['D'], fx['Gd'], chi[idx] * dJ[idx]),
         lc.ratio(tag, 'F', L.F[0], fx['F'], fx['Fg'], lc.FOUR_PI * (wabs @ dJ)),
         lc.ratio(tag, 'Q', L.Q[0], fx['Q'], fx['Qg'], lc.FOUR_PI * (wabs @ (chi * dJ))),
         lc.ratio(tag, 'Qt', L.Qt[0], fx['Qt'], fx['Qtg'], lc.qt_envelope(lc.qt_coefficients(prob, block, n[0], phi, wphi), dJ))]
    if (case, layout) == ('ca', 'compact'):
        flux_divergence_report(prob, block, L)
    assert max(r) <= 1.0, r


# ---- 2. a single 1 in the weights picks out one wavelength, bit for bit ---------------------------------------------------------------
def test_a_single_weight_gives_the_monochromatic_sums(hip_lib):
    prob, block, prof, n, J = lc.state('ca')
    e = hip_engine(hip_lib, prob, block, prof, n, J)
    full = e.radiative_losses(what=ALL)
    for la in (0, prob.Nspect // 2 + 3, prob.Nspect - 1):
        w = np.zeros(prob.Nspect)
        w[la] = 1.0
        L = e.radiative_losses(wnu=w, what=ALL)
        assert np.array_equal(L.wnu, w)
        assert np.array_equal(L.Q[0], lc.FOUR_PI * L.D[0, la]) and np.array_equal(L.F[0], lc.FOUR_PI * L.H[0, la])
        assert same_losses(L, full, fields=('Qt', 'H', 'D'))          # the weights touch F and Q alone
        assert np.any(L.Q[0] != 0) and np.any(L.F[0] != 0)
    e.close()


# ---- 3. made-up problems with vlos = 0: D = chi (S W - J), H at the top = sum wmu/2 mu I ---------------------------------------------
def identities(tag, oracle_lib, prob, blk, prof, e, solver):
    """the engine in the state under test -> the ratios of D and H[:, 0] to their bounds.  chi and S come from the depth-resolved
    final pass, J_pass and I from ONE formal solution of the same state (which this function runs last)"""
    n, Jd = e.get(LSX_N), e.get(LSX_J)
    before = snapshot(e)
    L = e.radiative_losses(what=ALL)
    assert same_losses(e.radiative_losses(what=ALL), L)              # nothing is accumulated over calls
    d = e.depth_rays([1.0], what=('chi', 'S'))
    assert same(snapshot(e), before)
    e.formal_sol_gamma()
    Jp, I = e.get(LSX_J), e.get(LSX_I)
    dJ, _ = lc.pass_envelope(oracle_lib, prob, blk, prof, n, Jd, solver)
    chi, S = (np.moveaxis(a[:, 0], -1, 1) for a in (d.chi, d.S))     # [ncol][Nspect][Nspace]
    W, hw, mu = lc.weight_sum(prob), lc.half_weights(prob), np.asarray(prob.muz)
    eta = S * chi
    rD = lc.ratio(tag, 'D', L.D, eta * W - chi * Jp, eta * W + chi * Jp, chi * dJ)
    top = np.einsum('m,clm->cl', hw * mu, I)
    rH = lc.ratio(tag, 'H[:, 0]', L.H[:, :, 0], top, top, dJ[:, :, 0])
    # what no bar is needed for: F and Q are the weighted sums of H and D to rounding, and |H| <= J max mu
    Fsum, Qsum = (lc.FOUR_PI * np.einsum('l,clk->ck', L.wnu, a) for a in (L.H, L.D))
    Fabs, Qabs = (lc.FOUR_PI * np.einsum('l,clk->ck', L.wnu, np.abs(a)) for a in (L.H, L.D))
    assert np.all(np.abs(L.F - Fsum) <= 4 * prob.Nspect * 2.0 ** -53 * Fabs) and np.all(np.abs(L.Q - Qsum) <= 4 * prob.Nspect * 2.0 ** -53 * Qabs)
    return L, max(rD, rH)


@pytest.mark.parametrize('name', lc.MADE_UP)
@pytest.mark.parametrize('solver', fp.SOLVERS)
def test_made_up_problems_meet_the_identities(hip_lib, oracle_lib, name, solver):
    prob, blk, prof, how = lc.made_up(name)
    assert prob.Nspect % 64 != 0
    if name in ('r1-sca', lc.FIVE_RAYS, 'deepest3-r7'):
        assert np.any(prob.active.sum(axis=0) == 0)               # a wavelength that no transition sees
    e = hip_engine(hip_lib, prob, blk, prof, solver=solver)
    if how == 'mali':
        rc.mali(e)
    else:
        e.formal_sol_gamma()
        e.formal_sol_gamma()
    L, r = identities('%s %s (%d rays, %d depths)' % (name, solver, prob.Nrays, prob.Nspace), oracle_lib, prob, blk, prof, e, solver)
    e.close()
    assert L.D.shape == (blk.ncol, prob.Nspect, prob.Nspace) and L.Qt.shape == (blk.ncol, prob.Ntrans, prob.Nspace)
    assert r <= 1.0


def test_the_made_up_table_covers_what_it_should():
    """(no GPU work) 1, 3, 5 and 7 rays -- with 7 the second group has two rays and adds to the first --, the three-depth column"""
    probs = {name: lc.made_up(name)[0] for name in lc.MADE_UP}
    assert sorted({p.Nrays for p in probs.values()}) == [1, 3, 5, 7]
    assert fp.walk_in_groups(7) == (5, 2) and probs['deepest3-r7'].Nspace == 3
    assert any(not p.phi_compact for p in probs.values())


# ---- 4. bits do not depend on how the work is cut -------------------------------------------------------------------------------------
@pytest.mark.parametrize('solver', fp.SOLVERS)
def test_losses_do_not_depend_on_how_the_columns_are_cut(hip_lib, solver):
    prob, block = fp.build(fp.SEVEN_COLUMNS)
    assert block.ncol == 7 and prob.Nrays == 11
    e = hip_engine(hip_lib, prob, block, None, solver=solver)
    rc.mali(e)
    whole = e.radiative_losses(what=ALL)
    for c0, nc in ((0, 3), (3, 4)):                                                # ranges of 3 + 4
        assert same_losses(e.radiative_losses(col0=c0, ncol=nc, what=ALL), whole, slice(c0, c0 + nc)), (c0, nc)
    per_col = 8 * prob.Nspace * (3 * prob.Nspect + 2 * prob.SNl)
    assert same_losses(e.radiative_losses(what=ALL, work_cap_bytes=2 * per_col + 64), whole)      # passes of 2 + 2 + 2 + 1 columns
    assert same_losses(e.radiative_losses(what=ALL, work_cap_bytes=1), whole)       # below one column's need: one column per pass
    assert same_losses(e.radiative_losses(col0=1, ncol=5, what=ALL, work_cap_bytes=2 * per_col + 64), whole, slice(1, 6))
    assert same_losses(e.radiative_losses(what=ALL, work_cap_bytes=0), whole)
    some = e.radiative_losses(what=('Q', 'D'))                                      # fewer outputs: the same bits
    assert some.F is None and some.Qt is None and some.H is None and same_losses(some, whole, fields=('Q', 'D'))
    n, J = e.get(LSX_N), e.get(LSX_J)
    e.close()
    shard = hip_engine(hip_lib, prob, block.slice(4, 7), None, n[4:7], J[4:7], solver=solver, policy_columns=7)
    assert same_losses(shard.radiative_losses(what=ALL), whole, slice(4, 7))        # a column's place in the context
    shard.close()


# ---- 5. read-only -------------------------------------------------------------------------------------------------------------------------
def test_the_call_changes_nothing(hip_lib):
    """a twin engine that never calls the entry gives bitwise the same I, J, Gamma, n and per-column monitors after the same script
    of calls -- including a call between a speculative formal solution and lsx_sync_end, and a discard afterwards"""
    ncol = 12
    prob, block, prof = rc.batch('falc_cah.npz', ncol)
    engines = [hip_engine(hip_lib, prob, block, prof) for _ in range(2)]
    probe, twin = engines
    seen = [probe.radiative_losses()]                             # before the first formal solution
    assert same(snapshot(probe), snapshot(twin))
    for it in range(4):
        for e in engines:
            e.formal_sol_gamma()
        seen.append(probe.radiative_losses(what=ALL))
        assert same(snapshot(probe), snapshot(twin))
        if it >= 2:
            for e in engines:
                e.stat_equil()
            seen.append(probe.radiative_losses(col0=1, ncol=ncol - 2))
            assert same(snapshot(probe), snapshot(twin))
    # the pipelined loop: FS; SE; sync_begin; speculative FS; [the call]; sync_end; discard
    for e in engines:
        e.formal_sol_gamma_async()
        e.stat_equil_async()
        e.sync_begin()
        e.formal_sol_gamma_speculative()
    spec = probe.radiative_losses()                # sees what lsx_get sees: the speculative call's J
    assert np.array_equal(probe.get(LSX_J), twin.get(LSX_J))
    mon = [e.sync_end() for e in engines]
    assert mon[0] == mon[1]
    assert same(snapshot(probe), snapshot(twin))
    for e in engines:
        e.discard_formal_sol()
    assert same(snapshot(probe), snapshot(twin))
    back = probe.radiative_losses()                # the accepted call's J again
    assert not np.array_equal(back.Q, spec.Q)
    for e in engines:                              # and the next two iterations produce the bits they would have produced
        e.formal_sol_gamma()
        e.stat_equil()
        e.formal_sol_gamma()
        e.stat_equil()
    assert same(snapshot(probe), snapshot(twin))
    for x in seen + [spec, back]:
        assert all(np.all(np.isfinite(getattr(x, f))) for f in ALL if getattr(x, f) is not None)
    for e in engines:
        e.close()


# ---- 6. frozen columns ----------------------------------------------------------------------------------------------------------------------
def test_frozen_columns_are_computed_like_any_other(hip_lib):
    prob, block = fp.build(fp.FROZEN)
    e = hip_engine(hip_lib, prob, block, None)
    rc.mali(e)
    L = e.radiative_losses(what=ALL)
    mask = np.array([True, False, True])
    e.set_active_columns(mask)
    assert same_losses(e.radiative_losses(what=ALL), L)
    e.formal_sol_gamma()                          # the frozen column keeps its J: its losses stay, the others move
    L2 = e.radiative_losses(what=ALL)
    for f in ALL:
        assert np.array_equal(getattr(L2, f)[~mask], getattr(L, f)[~mask]), f
    assert not np.array_equal(L2.Q[mask], L.Q[mask]) and not np.array_equal(L2.D[mask], L.D[mask])
    e.close()


# ---- 7. a refined grid ------------------------------------------------------------------------------------------------------------------------
def test_deep_columns(hip_lib, oracle_lib):
    """the 325-depth grid of tests/test_deep_columns.py, three columns, against the identities of the made-up problems: no depth limit"""
    fine, fblock = rt.refined('falc_cah.npz', 4, ncol=3)
    assert fine.phi_compact
    e = hip_engine(hip_lib, fine, fblock, None)
    rc.mali(e)
    L, r = identities('falc_cah x4 (325 depths)', oracle_lib, fine, fblock, None, e, 'linear')
    e.close()
    assert L.Q.shape == (3, 325) and r <= 1.0


# ---- 8. all five atoms --------------------------------------------------------------------------------------------------------------------------
def test_all_five_atoms_first_call(hip_lib):
    """109 transitions, up to 44 continua at one wavelength: everything finite, and a line's Qt is (hc / lambda_0) net() of
    lsx_hip_radiative_rates within the relative spread of the photon energy over the line's own grid, scaled by the gross
    (hc / lambda_0) (n_j Rji + n_i Rij)"""
    prob, block, raw = fixtures.load_problem_npz(golden('falc_all.npz'))
    assert prob.Ntrans == 109
    e = hip_engine(hip_lib, prob, block, None)
    L = e.radiative_losses(what=ALL)
    R = e.radiative_rates()
    n = e.get(LSX_N)[0]
    e.close()
    assert all(np.all(np.isfinite(getattr(L, f))) for f in ALL)
    assert np.array_equal(L.total()[0], L.Qt[0].sum(axis=0))
    worst, lines = 0.0, 0
    for kr, t in enumerate(prob.trans):
        if not t.is_line:
            continue
        lam = prob.wavelength[t.Nblue:t.Nblue + t.Nlambda]
        spread = float(np.max(np.abs(lam - t.lambda0)) / np.min(lam))          # |hc / lambda - hc / lambda_0| / (hc / lambda_0) at most
        o = int(prob.lev_off[t.atom])
        e0 = Const.HC / (t.lambda0 * Const.NM_TO_M)
        down, up = n[o + t.j] * R.Rji[0, kr], n[o + t.i] * R.Rij[0, kr]
        dev = np.abs(L.Qt[0, kr] - e0 * (down - up))
        bound = (spread + lc.BASE) * e0 * (down + up)
        worst = max(worst, float(np.max(dev / bound)))
        lines += 1
    print('falc_all: %d lines, Qt against (hc / lambda_0) net(): %.3f x the bound at worst' % (lines, worst))
    assert lines > 20 and worst <= 1.0


# ---- the drop-in side ---------------------------------------------------------------------------------------------------------------------------
def test_context_compute_losses(hip_lib):
    d = dict(np.load(golden('falc_ca.npz')))
    prob, block, raw = fixtures.load_problem_npz(golden('falc_ca.npz'))
    atmos, spect, eq, bg = build_fakes(d)
    ctx = Context(atmos, spect, eq, bg, lib=hip_lib)
    for it in range(4):
        ctx.formal_sol_gamma_matrices()
        if it >= 2:
            ctx.stat_equil()
    I_before, J_before = ctx.I.copy(), ctx.J.copy()
    L = ctx.compute_losses()
    assert not ctx._spec
    assert L.F.shape == L.Q.shape == (prob.Nspace,) and L.Qt.shape == (prob.Ntrans, prob.Nspace) and L.H is None and L.D is None
    assert L.transitions == [t for a in ctx.activeAtoms for t in a.trans] and len(L.transitions) == prob.Ntrans
    assert np.array_equal(L.wnu, lc.trapezoid_wnu(prob.wavelength)) and L.F[0] > 0
    assert np.array_equal(L.total(), L.Qt.sum(axis=0))
    t3 = L.transitions[3]
    assert np.array_equal(L.by_transition([t3])[t3], L.Qt[3]) and np.array_equal(L.by_transition(0)[0], L.Qt[0])
    # a band in nm: the trapezoid weights, zeroed outside -- and the two halves of the grid add up to the whole to rounding
    lam = prob.wavelength
    mid = 0.5 * (lam[prob.Nspect // 2] + lam[prob.Nspect // 2 + 1])
    lo, hi = ctx.compute_losses(wavelength_band=(0.0, mid), what=('F', 'Q', 'H', 'D')), ctx.compute_losses(wavelength_band=(mid, 1e9))
    assert np.array_equal(lo.wnu, np.where(lam <= mid, L.wnu, 0.0)) and np.array_equal(hi.wnu, np.where(lam >= mid, L.wnu, 0.0))
    assert np.array_equal(lo.wnu + hi.wnu, L.wnu) and lo.H.shape == (prob.Nspect, prob.Nspace)
    gross = lc.FOUR_PI * (L.wnu @ np.abs(lo.D))
    assert np.all(np.abs(lo.Q + hi.Q - L.Q) <= 4 * prob.Nspect * 2.0 ** -53 * gross)
    assert np.array_equal(hi.Qt, L.Qt)                    # Qt is summed over each transition's own wavelengths either way
    assert np.array_equal(ctx.I, I_before) and np.array_equal(ctx.J, J_before)
    again = ctx.compute_losses()
    assert all(np.array_equal(getattr(again, f), getattr(L, f)) for f in ('F', 'Q', 'Qt'))
    ctx.close()


# ---- 9. errors are found on the host ------------------------------------------------------------------------------------------------------------
def test_errors(hip_lib):
    prob, block, prof = rc.batch('falc_ca.npz', 4)
    e = Engine(prob, 4, lib=hip_lib)
    e.set_columns(0, block)                       # profiles not set yet
    with pytest.raises(_capi.LsxError) as err:
        e.radiative_losses()
    assert err.value.code == _capi.LSX_EINVAL and 'no line profiles' in str(err.value)
    e.set_line_profiles(0, *prof)
    e.formal_sol_gamma()
    before = snapshot(e)
    f = hip_lib.dll.lsx_hip_radiative_losses
    Ns, Nt, Nsp = prob.Nspace, prob.Ntrans, prob.Nspect
    out = [np.zeros((4, Ns)), np.zeros((4, Ns)), np.zeros((4, Nt, Ns)), np.zeros((4, Nsp, Ns)), np.zeros((4, Nsp, Ns))]
    nb = (out[0].nbytes, out[2].nbytes, out[3].nbytes)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def call(col0=0, ncol=4, wnu=None, ptrs=None, nbytes=nb, h=e._h):
        return f(h, col0, ncol, dp(wnu), *[dp(a) for a in (out if ptrs is None else ptrs)], *nbytes)
    assert call() == 0
    good = [x.copy() for x in out]
    assert all(np.all(np.isfinite(x)) and np.any(x != 0) for x in good)
    assert call(ptrs=(None,) * 5) == _capi.LSX_EINVAL
    assert call(col0=-1) == _capi.LSX_EINVAL
    assert call(col0=1, ncol=4) == _capi.LSX_EINVAL
    assert call(ncol=0) == _capi.LSX_EINVAL
    assert call(ncol=-2) == _capi.LSX_EINVAL
    assert call(ncol=3) == _capi.LSX_EINVAL                       # the byte counts are those of four columns
    for q in range(3):                                            # each byte count on its own
        bad = list(nb)
        bad[q] -= 8
        assert call(nbytes=tuple(bad)) == _capi.LSX_EINVAL
    for v in (np.nan, np.inf, -np.inf):                           # a weight that is not finite
        w = lc.trapezoid_wnu(prob.wavelength)
        w[Nsp // 3] = v
        assert call(wnu=w) == _capi.LSX_EINVAL
    assert call(h=None) == _capi.LSX_EINVAL
    assert all(np.array_equal(x, g) for x, g in zip(out, good)) and same(snapshot(e), before)     # nothing launched, nothing written
    # a byte count is looked at only where one of its outputs is asked for
    assert call(ptrs=(out[0], None, None, None, None), nbytes=(nb[0], 0, 0)) == 0
    # any subset of the outputs
    for keep in ((0,), (1,), (2,), (3,), (4,), (0, 2), (1, 3, 4)):
        for x in out:
            x[...] = 0.0
        assert call(ptrs=tuple(out[q] if q in keep else None for q in range(5))) == 0
        assert all(np.array_equal(out[q], good[q]) if q in keep else not out[q].any() for q in range(5))
    # negative weights are weights like any other
    assert call(wnu=-lc.trapezoid_wnu(prob.wavelength)) == 0
    assert np.array_equal(out[1], -good[1]) and np.array_equal(out[0], -good[0])
    # the Python side names what it does not know; the context is as usable as before
    with pytest.raises(ValueError):
        e.radiative_losses(what=('F', 'Gd'))
    with pytest.raises(ValueError):
        e.radiative_losses(wnu=np.ones(Nsp + 1))
    L = e.radiative_losses(what=ALL)
    assert all(np.array_equal(getattr(L, f), g) for f, g in zip(ALL, good))
    e.formal_sol_gamma()
    e.close()
