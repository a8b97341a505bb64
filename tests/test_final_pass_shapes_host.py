"""The cases of tests/final_pass_cases.py on the oracle alone: what keeps tests/test_final_pass_shapes.py honest.

The GPU tests hold the final-pass kernels to the FALC tests' bars, entry by entry and relative.  That says something only where every
entry is positive and its bound (BASE |x| + K_ENVELOPE |x(+1 ulp) - x(-1 ulp)|) is narrow, so both are asserted here for every case
under both rules, in the state the GPU tests evaluate it in (reached by the oracle): populations >= 0 with only the dead level at 0;
J, I and every rate finite and > 0; no bound wider than 1e-9 relative anywhere.  A case that cannot meet this is replaced.
Measured: the widest bound is 1.1e-11 relative for the rates, 8.7e-11 for the emergent rays (eight rays, compact, linear rule) and
3.6e-11 for the spectra."""
import numpy as np
import pytest

import envelope
import final_pass_cases as fp
import rates_cases as rt
import rays_cases as rc
import spectrum_cases as sc
from lightspinner_amd import _capi

LSX_I, LSX_J, LSX_N = _capi.LSX_I, _capi.LSX_J, _capi.LSX_N


def oracle_state(oracle_lib, prob, block, prof, case, solver):
    """-> (n, J, I) of the state the GPU tests evaluate the case in, reached by the oracle"""
    e = rt.oracle_engine(oracle_lib, prob, block, prof, solver=solver)
    fp.reach_state(e, case)
    out = e.get(LSX_N), e.get(LSX_J), e.get(LSX_I)
    e.close()
    return out


def positive(tag, **arrays):
    for k, a in arrays.items():
        assert np.all(np.isfinite(a)) and np.all(a > 0), '%s: %s is not finite and positive everywhere (smallest %.3e)' % (tag, k, np.min(a))


def widest(x0, env, base):
    """the largest bound relative to |x|"""
    return float(np.max((base * np.abs(x0) + envelope.K_ENVELOPE * env) / np.abs(x0)))


def check_populations(tag, prob, n, dead):
    assert np.all(np.isfinite(n)) and np.all(n >= 0), tag
    zero = np.nonzero(np.any(n == 0, axis=(0, 2)))[0].tolist()
    dead_level = [prob.NLtot - 1] if dead else []
    assert zero == dead_level or zero == [], '%s: levels %s hold a zero population' % (tag, zero)
    return zero


def test_the_table_reaches_every_rates_instance_as_a_first_and_as_a_later_group():
    seen = fp.check_group_coverage()
    assert len(seen) == 20
    for (nm, par, first), names in sorted(seen.items()):
        print('k_rates_pass<%d, %s> as %s group: %s' % (nm, 'parabolic' if par else 'linear', 'first' if first else 'a later', ', '.join(sorted(set(names)))))
    # the assertion notices a lost instance: these two cases are the only ones whose first group is of three / four rays
    for lost in ('r3-dead-level', 'r4-multiplet4'):
        with pytest.raises(AssertionError):
            fp.check_group_coverage([p for p in fp.RATES_PARAMS if p[0] != lost])


def test_the_table_covers_what_it_says():
    probs = {c.name: fp.build(c.name) for c in fp.CASES}
    assert sorted({p.Nrays for p, _ in probs.values()}) == [1, 2, 3, 4, 6, 7, 8, 9, 11, 64]
    assert {64 // p.Nrays for p, _ in probs.values()} == {64, 32, 21, 16, 10, 9, 8, 7, 5, 1}
    assert any(p.Nspect % (64 // p.Nrays) for p, _ in probs.values())                           # a ragged last tile
    deep = sorted({p.Nspace for p, _ in probs.values() if p.Nspace >= 20})
    assert all(20 <= k <= 45 for k in deep) and any(k % 2 for k in deep) and any(k % 2 == 0 for k in deep)
    assert sorted(p.Nspace for p, _ in probs.values() if p.Nspace < 20) == [3, 4, 5]
    assert all(fp.BY_NAME[name].state == ('two_fs' if p.Nspace < 20 else 'mali') for name, (p, _) in probs.items())
    assert sorted({b.ncol for _, b in probs.values()}) == [3, 7] and probs[fp.SEVEN_COLUMNS][1].ncol == 7
    assert probs[fp.SEVEN_COLUMNS][0].Nrays in (7, 11) and probs[fp.FROZEN][0].Nrays == 8
    assert all(p.Nspace <= 45 and p.Nspect <= 150 and b.ncol <= 7 for p, b in probs.values())
    assert {p.phi_compact for p, _ in probs.values()} == {True, False} and any(p.sca_per_lambda for p, _ in probs.values())
    assert any(all(t.is_line for t in p.trans) for p, _ in probs.values())                      # no continua: E and nsr are NULL
    assert any(sum(t.is_line for t in p.trans) == 4 for p, _ in probs.values())                 # a multiplet of four
    assert [p.Nrays for p, _ in (probs[q] for q in fp.QUADRATURE)] == [1, 7, 8, 64]
    p7, p8, p1 = (probs[name][0] for name, _ in fp.DEPTH)
    assert (p7.Nrays, p7.phi_compact) == (7, False) and (p8.Nrays, p8.phi_compact) == (8, True) and (p1.Nrays, p1.sca_per_lambda) == (1, True)
    assert fp.DEPTH[0][1] == fp.SOLVERS


@pytest.mark.parametrize('name,solver', fp.RATES_PARAMS)
def test_rates_cases_are_well_posed(oracle_lib, name, solver):
    case = fp.BY_NAME[name]
    prob, block = fp.build(name)
    tag = '%s %s' % (name, solver)
    n, J, I = oracle_state(oracle_lib, prob, block, None, case, solver)
    zero = check_populations(tag, prob, n, 'dead' in name)
    if 'dead' in name:
        assert zero == [prob.NLtot - 1]                            # the statistical equilibrium drove it to 0 exactly
    positive(tag + ' state', J=J, I=I)
    runs = rt.oracle_runs(oracle_lib, prob, block, None, n, J, solver)
    r = runs[0][0]
    positive(tag + ' rates pass', Rij=r[rt.RIJ], Rji=r[rt.RJI], Rji_ref=r[rt.RJI_REF], J=r[LSX_J])
    wide = max(widest(r[w], envelope.envelope(runs, 0, w), rt.BASE) for w in (rt.RIJ, rt.RJI, rt.RJI_REF))
    # the oracle agrees with itself: a continuum's Rij is the restatement from the J of the same pass
    worst = 0.0
    for kr, t in enumerate(prob.trans):
        if not t.is_line:
            mine = rt.continuum_rates(prob, block, kr, r[LSX_J])[0]
            worst = max(worst, float(np.max(np.abs(mine - r[rt.RIJ][:, kr]) / r[rt.RIJ][:, kr])))
    print('%s: widest rates bound %.2e relative; continuum restatement against the oracle %.1e' % (tag, wide, worst))
    assert wide <= fp.VACUITY_CAP
    assert worst <= 1e-13


@pytest.mark.parametrize('name,solver', fp.RATES_PARAMS)
def test_rays_cases_are_well_posed(oracle_lib, name, solver):
    """the context the emergent-ray tests load (compact arrays, or profiles the library builds from made-up inputs)"""
    case = fp.BY_NAME[name]
    prob, block = fp.build(name)
    blk, prof = fp.rays_inputs(prob, block)
    tag = '%s %s' % (name, solver)
    n, J, I = oracle_state(oracle_lib, prob, blk, prof, case, solver)
    check_populations(tag, prob, n, 'dead' in name)
    positive(tag + ' state', J=J, I=I)
    runs = rc.envelope_runs(oracle_lib, prob, blk, prof, rc.MUS20, n, J, solver)
    positive(tag + ' rays', I=runs[0][0][LSX_I])
    wide = widest(runs[0][0][LSX_I], envelope.envelope(runs, 0, LSX_I), 1e-11)
    if name in fp.QUADRATURE:
        own = rc.envelope_runs(oracle_lib, prob, blk, prof, prob.muz, n, J, solver)
        positive(tag + ' quadrature angles', I=own[0][0][LSX_I])
        wide = max(wide, widest(own[0][0][LSX_I], envelope.envelope(own, 0, LSX_I), 1e-11))
    print('%s: widest rays bound %.2e relative' % (tag, wide))
    assert wide <= fp.VACUITY_CAP


@pytest.mark.parametrize('name,solver', [(name, s) for name, rules in fp.SPECTRUM for s in rules])
def test_spectrum_cases_are_well_posed(oracle_lib, name, solver):
    case = fp.BY_NAME[name]
    prob, block = fp.build(name)
    blk, prof = fp.library_profiles(prob, block)
    tag = '%s %s' % (name, solver)
    n, J, I = oracle_state(oracle_lib, prob, blk, prof, case, solver)
    check_populations(tag, prob, n, False)
    positive(tag + ' state', J=J, I=I)
    w = fp.made_up_wanted(prob)
    alpha, bg = sc.interp_alpha(prob, w), fp.given_background(prob, block, w)
    assert (alpha is None) == (name == 'lines-only') and len(bg) == (3 if prob.sca_per_lambda else 2)
    mus = rc.MUS20[::4]
    wide = 0.0
    for mode, given in (('handed over', bg), ('interpolated', None)):
        x0, xp, xm = sc.envelope_spectrum(oracle_lib, prob, blk, prof, mus, n, J, w, alpha, given, solver)
        positive('%s spectrum, background %s' % (tag, mode), I=x0)
        wide = max(wide, float(np.max(sc.bound(x0, xp, xm) / np.abs(x0))))
    print('%s: widest spectrum bound %.2e relative' % (tag, wide))
    assert wide <= fp.VACUITY_CAP


def test_a_thin_slab_at_the_top_is_what_the_shallow_cases_avoid(oracle_lib):
    """toy_problem(Nspace=3) under the linear rule: the mean intensity changes sign -- the reason the shallow cases are the deepest
    points of a 37-depth column.  The well-posedness checks above fail on it."""
    from toy import toy_problem
    prob, block = toy_problem(seed=42, Nspace=3, Nrays=7, Nspect=60)
    n, J, I = oracle_state(oracle_lib, prob, block, None, fp.BY_NAME['deepest3-r7'], 'linear')
    with pytest.raises(AssertionError):
        positive('Nspace=3', J=J, I=I)
