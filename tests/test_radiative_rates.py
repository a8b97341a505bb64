"""Radiative rates from a converged context on the GPU (include/lsx_hip_rates.h, lsx_hip_radiative_rates; Engine.radiative_rates,
Context.compute_rates) against the reference's own first-call rates (tests/golden/falc_*.npz: fs1_Rij_t*, fs1_Rji_t*) and against
the oracle (tests/rates_cases.py).

The bars are the project's rule for one formal solution, no new numbers: against the oracle every entry inside 1e-11 |x| + 3 x what
a one-ulp change of the oracle's own exp() does to that entry (tests/envelope.py); against the reference that plus what the oracle
itself is away from the reference on the case (the rule of tests/test_emergent_rays.py).  Rates are sums of non-negative terms, so
the bars hold entry by entry.  Every call here is an ordinary valid call or is refused on the host."""
import ctypes as C

import numpy as np
import pytest

import envelope
import rates_cases as rt
import rays_cases as rc
from conftest import golden
from helpers import build_fakes
from lightspinner_amd import _capi, drivers, fixtures, synth
from lightspinner_amd.problem import Engine, RadiativeRates
from lightspinner_amd.rh_method import Context

pytestmark = pytest.mark.gpu
WHAT = (rt.RIJ, rt.RJI_REF, rt.RJI)


def hip_engine(hip_lib, prob, block, prof, n=None, J=None, solver='linear', **kw):
    e = Engine(prob, block.ncol, lib=hip_lib, **kw)
    synth.load_columns(e, block, prof)
    e.set_formal_solver(solver)
    if n is not None:
        e.set(_capi.LSX_N, n)
    if J is not None:
        e.set(_capi.LSX_J, J)
    return e


def as_dict(r):
    return {rt.RIJ: r.Rij, rt.RJI_REF: r.Rji_ref, rt.RJI: r.Rji}


def inside_oracle(tag, r, runs, what=WHAT):
    """every entry of the three rates inside the oracle's envelope; prints deviation and envelope per array"""
    got = as_dict(r)
    for w in what:
        assert got[w].shape == runs[0][0][w].shape and np.all(np.isfinite(got[w]))
        rt.report(tag, got[w], runs, w)
    for w in what:
        envelope.inside(got[w], runs, 0, w, base=rt.BASE)


# ---- 1. the first call: the reference's own numbers ------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(rt.GOLDEN_FIXTURES))
def test_a_fresh_engine_gives_the_reference_first_call(hip_lib, oracle_lib, case):
    prob, block, raw = fixtures.load_problem_npz(golden(rt.GOLDEN_FIXTURES[case]))
    e = hip_engine(hip_lib, prob, block, None)                     # no formal solution yet: J = 0, LTE populations
    r = e.radiative_rates()
    e.close()
    assert r.Rij.shape == r.Rji.shape == r.Rji_ref.shape == (1, prob.Ntrans, prob.Nspace)
    runs = rt.oracle_runs(oracle_lib, prob, block)
    inside_oracle('%s first call against the oracle' % case, r, runs)
    for mine, w, ref in zip((r.Rij[0], r.Rji_ref[0]), (rt.RIJ, rt.RJI_REF), rt.golden_rates(raw, prob)):
        x0, env = runs[0][0][w][0], envelope.envelope(runs, 0, w)[0]
        dref = float(np.max(np.abs(x0 - ref) / ref))
        assert dref <= rt.GOLDEN_BAR
        bound = dref * np.abs(ref) + rt.BASE * np.abs(x0) + envelope.K_ENVELOPE * env
        dev = np.abs(mine - ref)
        print('%s %s against the reference: largest deviation %.2e relative (oracle against the reference %.1e), %.3f x the bound'
              % (case, w, np.max(dev / ref), dref, np.max(dev / bound)))
        assert np.all(dev <= bound)


def test_all_five_atoms_first_call_meets_the_oracle(hip_lib, oracle_lib):
    """109 transitions, up to 44 continua at one wavelength"""
    prob, block, raw = fixtures.load_problem_npz(golden('falc_all.npz'))
    assert prob.Ntrans == 109
    e = hip_engine(hip_lib, prob, block, None)
    r = e.radiative_rates()
    e.close()
    inside_oracle('falc_all first call', r, rt.oracle_runs(oracle_lib, prob, block))


# ---- 2. + 4. later states against the oracle, the physical Rji among them ----------------------------------------------------------
@pytest.mark.parametrize('case', ['ca', 'cah', 'ca_vlos', 'ca_vlos_arrays'])
def test_later_states_meet_the_oracle(hip_lib, oracle_lib, case):
    """lines: Rji against Rji_ref + (gij - 1) Rij of the oracle, continua against the restatement from the oracle's J (rates_cases)"""
    prob, block, prof, n, J = rt.later_state(case.replace('_arrays', ''))
    e = hip_engine(hip_lib, prob, block, prof, n, J)
    if case == 'ca_vlos_arrays':                   # the 4-D profiles handed over through lsx_set_columns: no kept profile inputs
        assert not prob.phi_compact
        block, prof = rt.with_profile_arrays(e, block), None
        assert block.phi.shape == (1,) + prob.phi_shape() and len(prob.phi_shape()) == 4
        built = e.radiative_rates()
        e.close()
        e = hip_engine(hip_lib, prob, block, None, n, J)
    r = e.radiative_rates()
    if case == 'ca_vlos_arrays':                   # the same numbers in the store, whoever put them there
        assert all(np.array_equal(a, b) for a, b in zip((r.Rij, r.Rji, r.Rji_ref), (built.Rij, built.Rji, built.Rji_ref)))
    e.close()
    inside_oracle('%s later state' % case, r, rt.oracle_runs(oracle_lib, prob, block, prof, n, J))


def test_context_compute_rates_closes_the_rate_equations(hip_lib, oracle_lib):
    """the drop-in Context after the 46-iteration FALC CaII loop (test.py:20-29): .transitions, .net(), and the rate equations close
    with the physical Rji as well as the oracle's rates of the same state do (+ 1e-9)"""
    d = dict(np.load(golden('falc_ca.npz')))
    prob, block, raw = fixtures.load_problem_npz(golden('falc_ca.npz'))
    atmos, spect, eq, bg = build_fakes(d)
    ctx = Context(atmos, spect, eq, bg, lib=hip_lib)
    h = drivers.iterate_mali(ctx)
    assert h.converged and h.n_iter == 46
    I_before, J_before = ctx.I.copy(), ctx.J.copy()
    r = ctx.compute_rates()
    assert not ctx._spec
    assert r.Rij.shape == r.Rji.shape == r.Rji_ref.shape == (prob.Ntrans, prob.Nspace)
    assert r.transitions == [t for a in ctx.activeAtoms for t in a.trans] and len(r.transitions) == prob.Ntrans
    n = np.concatenate([a.n for a in ctx.activeAtoms])
    net = r.net()
    for kr, t in enumerate(r.transitions):
        assert np.array_equal(net[kr], t.atom.n[t.j] * r.Rji[kr] - t.atom.n[t.i] * r.Rij[kr])
        assert not hasattr(t, 'Rij') and not hasattr(t, 'Rji')
    assert np.array_equal(ctx.I, I_before) and np.array_equal(ctx.J, J_before)
    runs = rt.oracle_runs(oracle_lib, prob, block, None, n[None], J_before[None])
    inside_oracle('Context after the loop', RadiativeRates(r.Rij[None], r.Rji[None], r.Rji_ref[None]), runs)
    miss = rt.closure(prob, block, n, r.Rij, r.Rji)
    miss_o = rt.closure(prob, block, n, runs[0][0][rt.RIJ][0], runs[0][0][rt.RJI][0])
    print('closure after the loop: HIP %.3e, oracle %.3e; with the reference form %.2e'
          % (miss.max(), miss_o.max(), rt.closure(prob, block, n, r.Rij, r.Rji_ref).max()))
    assert miss.max() <= miss_o.max() + 1e-9 and miss_o.max() <= 2e-3
    assert rt.closure(prob, block, n, r.Rij, r.Rji_ref).max() > 0.05
    # a second call is the same computation; the loop goes on as if nothing had happened
    again = ctx.compute_rates()
    assert all(np.array_equal(getattr(again, k), getattr(r, k)) for k in ('Rij', 'Rji', 'Rji_ref'))
    ctx.close()


# ---- 3. batches against the oracle --------------------------------------------------------------------------------------------------
BATCHES = [(f, p, nc, s) for f in ('falc_ca.npz', 'falc_cah.npz') for p, nc in (('ray-per-lane', 41), ('ray-serial', 160))
           for s in ('linear', 'parabolic')]


@pytest.mark.parametrize('fixture,policy,ncol,solver', BATCHES)
def test_batches_after_mali_iterations_meet_the_oracle(hip_lib, oracle_lib, fixture, policy, ncol, solver):
    """FALC-perturbed columns with a line-of-sight velocity, five MALI iterations under either sweep mapping; the oracle works on the
    HIP engine's own n and J, column by column"""
    prob, block, prof = rc.batch(fixture, ncol)
    e = hip_engine(hip_lib, prob, block, prof, solver=solver, sweep_policy=policy)
    if solver == 'linear':
        assert e.sweep_policy() == policy
    rc.mali(e)
    n, J = e.get(_capi.LSX_N), e.get(_capi.LSX_J)
    r = e.radiative_rates()
    part = e.radiative_rates(col0=7, ncol=20)                      # a sub-range of the columns is the same computation
    e.close()
    assert all(np.array_equal(getattr(part, k), getattr(r, k)[7:27]) for k in ('Rij', 'Rji', 'Rji_ref'))
    runs = rt.oracle_runs(oracle_lib, prob, block, prof, n, J, solver)
    inside_oracle('%s %s %s %d columns' % (fixture, policy, solver, ncol), r, runs)


# ---- 5. read-only -------------------------------------------------------------------------------------------------------------------
def snapshot(e):
    return {w: e.get(w) for w in (_capi.LSX_I, _capi.LSX_J, _capi.LSX_GAMMA, _capi.LSX_N, _capi.LSX_DJ_COL, _capi.LSX_DPOPS_COL)}


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def same_rates(a, b, cols=slice(None)):
    return all(np.array_equal(getattr(a, k), getattr(b, k)[cols]) for k in ('Rij', 'Rji', 'Rji_ref'))


@pytest.mark.parametrize('ncol,policy', [(12, 'auto'), (165, 'ray-serial')])
def test_the_call_changes_nothing(hip_lib, ncol, policy):
    """a twin engine that never calls the entry gives bitwise the same I, J, Gamma, n and per-column monitors after the same script
    of calls -- including a call between a speculative formal solution and lsx_sync_end, and a discard afterwards"""
    prob, block, prof = rc.batch('falc_cah.npz', ncol)
    engines = [hip_engine(hip_lib, prob, block, prof, sweep_policy=policy) for _ in range(2)]
    probe, twin = engines
    seen = [probe.radiative_rates()]                              # before the first formal solution
    assert same(snapshot(probe), snapshot(twin))
    for it in range(4):
        for e in engines:
            e.formal_sol_gamma()
        seen.append(probe.radiative_rates())
        assert same(snapshot(probe), snapshot(twin))
        if it >= 2:
            for e in engines:
                e.stat_equil()
            seen.append(probe.radiative_rates(col0=1, ncol=ncol - 2))
            assert same(snapshot(probe), snapshot(twin))
    # the pipelined loop: FS; SE; sync_begin; speculative FS; [the call]; sync_end; discard
    for e in engines:
        e.formal_sol_gamma_async()
        e.stat_equil_async()
        e.sync_begin()
        e.formal_sol_gamma_speculative()
    spec = probe.radiative_rates()                 # sees what lsx_get sees: the speculative call's J
    assert np.array_equal(probe.get(_capi.LSX_J), twin.get(_capi.LSX_J))
    mon = [e.sync_end() for e in engines]
    assert mon[0] == mon[1]
    assert same(snapshot(probe), snapshot(twin))
    for e in engines:
        e.discard_formal_sol()
    assert same(snapshot(probe), snapshot(twin))
    back = probe.radiative_rates()                 # the accepted call's J again
    assert not np.array_equal(back.Rij, spec.Rij)
    for e in engines:                              # and the next two iterations produce the bits they would have produced
        e.formal_sol_gamma()
        e.stat_equil()
        e.formal_sol_gamma()
        e.stat_equil()
    assert same(snapshot(probe), snapshot(twin))
    for x in seen + [spec, back]:
        assert all(np.all(np.isfinite(v)) and np.all(v > 0) for v in (x.Rij, x.Rji, x.Rji_ref))
    for e in engines:
        e.close()


def test_frozen_columns_are_computed_like_any_other(hip_lib):
    prob, block, prof = rc.batch('falc_ca.npz', 20)
    probe, twin = (hip_engine(hip_lib, prob, block, prof) for _ in range(2))
    for e in (probe, twin):
        rc.mali(e)
    r = probe.radiative_rates()
    mask = np.arange(20) % 3 != 0
    for e in (probe, twin):
        e.set_active_columns(mask)
    assert same_rates(probe.radiative_rates(), r)
    for e in (probe, twin):
        e.formal_sol_gamma()                      # the frozen columns keep their J: their rates stay, the others move
    r2 = probe.radiative_rates()
    assert np.array_equal(r2.Rij[~mask], r.Rij[~mask]) and not np.array_equal(r2.Rij[mask], r.Rij[mask])
    for e in (probe, twin):
        e.stat_equil()
        e.formal_sol_gamma()
    assert same(snapshot(probe), snapshot(twin))
    probe.close()
    twin.close()


# ---- 6. reproducibility ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('solver', ['linear', 'parabolic'])
def test_rates_do_not_depend_on_how_the_columns_are_split_or_chunked(hip_lib, solver):
    N = 41
    prob, block, prof = rc.batch('falc_cah.npz', N)
    whole = hip_engine(hip_lib, prob, block, prof, solver=solver, policy_columns=N)
    rc.mali(whole)
    r = whole.radiative_rates()
    assert same_rates(whole.radiative_rates(), r)                                  # two calls
    assert same_rates(whole.radiative_rates(col0=13, ncol=9), r, slice(13, 22))    # a column range
    # a work cap that holds three columns: 14 passes instead of one, the same bits; and back to the default
    per_col = 8 * prob.Nspace * (prob.Nspect + 2 * prob.SNl)
    assert same_rates(whole.radiative_rates(work_cap_bytes=3 * per_col + 64), r)
    assert same_rates(whole.radiative_rates(work_cap_bytes=1), r)                  # below one column's need: one column per pass
    assert same_rates(whole.radiative_rates(work_cap_bytes=0), r)
    n, J = whole.get(_capi.LSX_N), whole.get(_capi.LSX_J)
    whole.close()
    for c0, c1 in ((0, 20), (20, 41)):                                             # the same columns as 20 + 21
        sl = tuple(x[c0:c1] for x in prof)
        shard = hip_engine(hip_lib, prob, block.slice(c0, c1), sl, n[c0:c1], J[c0:c1], solver=solver, policy_columns=N)
        assert same_rates(shard.radiative_rates(), r, slice(c0, c1)), (c0, c1)
        shard.close()


# ---- 7. a refined grid ----------------------------------------------------------------------------------------------------------------
def test_deep_columns(hip_lib, oracle_lib):
    """the 325-depth grid of tests/test_deep_columns.py, three columns: no depth limit"""
    fine, fblock = rt.refined('falc_cah.npz', 4, ncol=3)
    e = hip_engine(hip_lib, fine, fblock, None)
    rc.mali(e)
    n, J = e.get(_capi.LSX_N), e.get(_capi.LSX_J)
    r = e.radiative_rates()
    e.close()
    inside_oracle('falc_cah x4 (325 depths)', r, rt.oracle_runs(oracle_lib, fine, fblock, None, n, J))


# ---- 8. errors are found on the host ----------------------------------------------------------------------------------------------------
def test_errors(hip_lib):
    prob, block, prof = rc.batch('falc_ca.npz', 4)
    e = Engine(prob, 4, lib=hip_lib)
    e.set_columns(0, block)                       # profiles not set yet
    with pytest.raises(_capi.LsxError) as err:
        e.radiative_rates()
    assert err.value.code == _capi.LSX_EINVAL and 'no line profiles' in str(err.value)
    e.set_line_profiles(0, *prof)
    e.formal_sol_gamma()
    before = snapshot(e)
    f = hip_lib.dll.lsx_hip_radiative_rates
    out = [np.zeros((4, prob.Ntrans, prob.Nspace)) for _ in range(3)]
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def call(col0=0, ncol=4, nbytes=None, ptrs=None):
        a, b, c = out if ptrs is None else ptrs
        return f(e._h, col0, ncol, dp(a), dp(b), dp(c), out[0].nbytes if nbytes is None else nbytes)
    assert call() == 0
    good = [x.copy() for x in out]
    assert all(np.all(x > 0) for x in good)
    assert call(ptrs=(None, None, None)) == _capi.LSX_EINVAL
    assert call(col0=-1) == _capi.LSX_EINVAL
    assert call(col0=1, ncol=4) == _capi.LSX_EINVAL
    assert call(ncol=0) == _capi.LSX_EINVAL
    assert call(ncol=-2) == _capi.LSX_EINVAL
    assert call(nbytes=out[0].nbytes - 8) == _capi.LSX_EINVAL
    assert call(ncol=3) == _capi.LSX_EINVAL                       # nbytes_each is that of four columns
    assert f(None, 0, 4, dp(out[0]), dp(out[1]), dp(out[2]), out[0].nbytes) == _capi.LSX_EINVAL
    assert all(np.array_equal(x, g) for x, g in zip(out, good)) and same(snapshot(e), before)     # nothing launched, nothing written
    # any one or two of the outputs
    for keep in ((0,), (1,), (2,), (0, 2)):
        for x in out:
            x[...] = 0.0
        assert call(ptrs=tuple(out[q] if q in keep else None for q in range(3))) == 0
        assert all(np.array_equal(out[q], good[q]) if q in keep else not out[q].any() for q in range(3))
    # the context is as usable as before
    assert same_rates(e.radiative_rates(), RadiativeRates(*[good[q] for q in (0, 1, 2)]))
    e.formal_sol_gamma()
    e.close()
    # ray-dependent profiles handed over as arrays are served (tests above); so are a phi_compact context's
    prob, base, raw = fixtures.load_problem_npz(golden('falc_ca.npz'))
    assert prob.phi_compact
    e = Engine(prob, 1, lib=hip_lib)
    e.set_columns(0, base)
    assert np.all(e.radiative_rates().Rij > 0)
    e.close()
