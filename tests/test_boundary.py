"""The radiation boundary conditions on the GPU (include/lsx_hip_boundary.h): zero, thermalised or given at both ends of a column.

The reference is its own Gamma loop with the start value of the rays replaced (tests/golden/boundary_*.npz, tests/boundary_cases.py,
tests/golden/make_boundary_golden.py).  The bars:
  Gamma        conftest.gamma_err under the project's bars of tests/topology_reference.py: off-diagonal < 1e-10, diagonal < 1e-11;
  I, J         entry by entry, envelope.excess with the fixture as the centre, TOL = 1e-11 on scale = |x_def| + |x - x_def| and
               K_ENVELOPE x the oracle's one-ulp-exp envelope under the DEFAULT boundary.  The solution is linear in the start
               value, x = x_def + dI_start T (same J-dagger: the oracle's second call is given the fixture's J of call 1): the
               rounding of the first part is what the default bar allows, the second is a product of Nspace factors e^-dtau, Nspace
               ulps relative -- far below TOL;
  rates        GOLDEN_BAR |ref| + BASE (|x_def| + |ref - x_def|) + K_ENVELOPE env_def, constants of tests/rates_cases.py.
The tests that compare the library with itself ask for identical bits."""
import numpy as np
import pytest

import boundary_cases as bc
import envelope
import rates_cases as rt
import topology_cases as tc
import topology_reference as tr
from conftest import gamma_err
from lightspinner_amd import _capi
from lightspinner_amd.problem import ColumnBlock, Engine
from toy import toy_problem

pytestmark = pytest.mark.gpu

# the context of the arbitrary-angle tests: ray-independent profiles (the final passes serve a compact context's own arrays as they
# are), eight rays, unchained continua -- tests/final_pass_cases.py, 'r8-compact'
ANGLES = dict(seed=37, Nrays=8, Nspace=30, Nspect=90, chain=False, phi_compact=True)

I_, J_, G_, DJ_ = _capi.LSX_I, _capi.LSX_J, _capi.LSX_GAMMA, _capi.LSX_DJ_COL
TOL = 1e-11


def _ncol(name):
    kind, arg = tc.TABLE[name]
    return arg.get('ncol', 3) if kind == 'toy' else arg[1] if kind == 'inst' else arg


def _has_ray_serial(name):
    kind, arg = tc.TABLE[name]
    return kind != 'toy' or (arg.get('Nrays', 3) == 5 and not arg.get('sca_per_lambda', False))


def _policies(name):
    if _ncol(name) < 32:
        return ('auto',)
    return ('ray-per-lane', 'ray-serial') if _has_ray_serial(name) else ('ray-per-lane',)


_built = {}


def _case(name):
    """(prob, block, golden columns, the golden columns as a block) -- no fixture of the topology family is needed"""
    if name not in _built:
        prob, block = tc.build(name)
        cols = tc.golden_columns(name, block.ncol)
        _built[name] = (prob, block, cols, ColumnBlock.concatenate([block.slice(c, c + 1) for c in cols]))
    return _built[name]


_def_runs = {}


def _default_runs(oracle_lib, name, combo, J1):
    """the oracle under the DEFAULT boundary on the golden columns, as it is and with every exp(-dtau) a ulp up / down: call 1 from
    J-dagger = 0, call 2 from the fixture's J of call 1 under `combo` (the J-dagger of the run that is checked)"""
    if (name, combo) not in _def_runs:
        prob, _, _, sub = _case(name)
        out = {}
        try:
            for ulp in (0, 1, -1):
                oracle_lib.dll.lsx_oracle_set_exp_ulp(int(ulp))
                e = Engine(prob, sub.ncol, lib=oracle_lib)
                e.set_columns(0, sub)
                oracle_lib.dll.lsx_oracle_set_threads(e._h, 8)
                snaps = []
                with np.errstate(all='ignore'):
                    e.formal_sol_gamma()
                    snaps.append({w: e.get(w) for w in (I_, J_)})
                    e.set(J_, J1)
                    e.formal_sol_gamma()
                    snaps.append({w: e.get(w) for w in (I_, J_)})
                e.close()
                out[ulp] = snaps
        finally:
            oracle_lib.dll.lsx_oracle_set_exp_ulp(0)
        _def_runs[(name, combo)] = out
    return _def_runs[(name, combo)]


def _two_calls(e, cols):
    snaps = []
    with np.errstate(all='ignore'):
        for _ in range(2):
            e.formal_sol_gamma()
            snaps.append({w: e.get(w)[cols] for w in (I_, J_, G_, DJ_)})
    return snaps


RUNS5 = [(n, cb, p) for n in bc.CASES for cb in bc.COMBOS for p in _policies(n)]


@pytest.mark.parametrize('name,combo,policy', RUNS5, ids=['%s-%s-%s' % r for r in RUNS5])
def test_hip_meets_the_reference_loop(hip_lib, oracle_lib, name, combo, policy):
    """5: every case x combination, on the mapping the case is meant for and with the policy forcing the other where it can run"""
    prob, block, cols, _ = _case(name)
    ref = bc.results(name, combo, cols)
    for c, dg in zip(cols, ref['digest']):
        assert np.array_equal(dg, tc.input_digest(prob, block, c))
    e = Engine(prob, block.ncol, lib=hip_lib, sweep_policy=policy)
    e.set_columns(0, block)
    bc.set_on(e, combo, prob, block)
    assert np.array_equal(e.boundary_state(), np.tile(np.array(bc.kinds(combo), dtype=np.int32), (block.ncol, 1)))
    snaps = _two_calls(e, np.asarray(cols))
    e.close()
    dflt = _default_runs(oracle_lib, name, combo, ref['fs1_J'])
    eps_prev = np.zeros(len(cols))
    for it, s in enumerate(snaps):
        tag = 'fs%d_' % (it + 1)
        off, diag = gamma_err(s[G_], ref[tag + 'Gamma'], prob)
        print('%s %s %s call %d: Gamma off %.2e diag %.2e' % (name, combo, policy, it + 1, off, diag), end='')
        runs = {0: [None, None], 1: dflt[1], -1: dflt[-1]}
        ratios = {}
        for w, key in ((I_, tag + 'I'),) + (((J_, tag + 'J'),) if it == 0 else ()):
            runs[0][it] = {w: ref[key]}
            x_def = dflt[0][it][w]
            scale = np.abs(x_def) + np.abs(ref[key] - x_def)
            ratios[w] = envelope.excess(s[w], runs, it, w, TOL, scale=scale)
            print('  %s %.3g x its bar (%.2e relative)' % ('I' if w == I_ else 'J', ratios[w][0], ratios[w][1]), end='')
        print()
        assert off < 1e-10 and diag < 1e-11, (name, combo, policy, it, off, diag)
        for w, r in ratios.items():
            assert r[0] <= 1.0, (name, combo, policy, it, w, r)
        if it == 0:
            eps = tr._column_dev(s[J_], ref['fs1_J'])
        else:       # J of call 2 is not kept: the single-call bound with the default runs' envelope, on the same scale as above
            J0 = np.abs(dflt[0][1][J_])
            with np.errstate(all='ignore'):
                b = TOL + envelope.K_ENVELOPE * np.where(J0 > 0, envelope.envelope(dflt, 1, J_) / J0, 0.0)
            eps = b.reshape(b.shape[0], -1).max(axis=1)
        r = tr._monitor_ratio(s[DJ_], ref[tag + 'dJ'], np.maximum(eps, eps_prev))
        assert r <= 1.0, (name, combo, policy, it, 'dJ per column', r, s[DJ_], ref[tag + 'dJ'])
        eps_prev = eps


@pytest.mark.parametrize('name', ['rs-see13-Nra5-Nsp41-Nsp120-nco34-mul3', 'toy-see7-Nra8-Nsp21-Nsp48-nco2'])
@pytest.mark.parametrize('graph', [False, True], ids=['launches', 'captured-graph'])
def test_default_is_untouched(hip_lib, name, graph):
    """6: never set / set explicitly to (thermalised, zero) / set to GG and back: identical bits over two calls; the third context's
    boundary changes twice between calls and each change shows in the next call (also through a captured graph)"""
    prob, block, _, _ = _case(name)
    opts = 'graph=1' if graph else None

    def make():
        e = Engine(prob, block.ncol, lib=hip_lib, options=opts)
        e.set_columns(0, block)
        return e

    def calls(e, n=2):
        out = []
        with np.errstate(all='ignore'):
            for _ in range(n):
                e.formal_sol_gamma()
                out.append([e.get(w) for w in (I_, J_, G_)])
        return out
    a = make()
    ra = calls(a)
    assert np.array_equal(a.boundary_state(), np.tile(np.array([bc.THERMALISED, bc.ZERO], dtype=np.int32), (block.ncol, 1)))
    a.close()
    b = make()
    b.set_boundary('thermalised', 'zero')
    rb = calls(b)
    b.close()
    # GG from the start: what the detour of the third context has to show
    g = make()
    bc.set_on(g, 'GG', prob, block)
    rg = calls(g, 1)
    g.close()
    c = make()
    rc = calls(c, 1)                               # default (captures the graph with a null boundary)
    bc.set_on(c, 'GG', prob, block)
    c.set(J_, np.zeros_like(rc[0][1]))
    rcg = calls(c, 1)                              # ... GG from J-dagger = 0: the call of context g
    c.set_boundary('thermalised', 'zero')
    c.set(J_, rc[0][1])
    rc += calls(c, 1)                              # ... and back: call 2 of the default sequence
    c.close()
    for x, y in zip(ra, rb):
        for u, v in zip(x, y):
            assert np.array_equal(u, v, equal_nan=True)
    for x, y in zip(ra, rc):
        for u, v in zip(x, y):
            assert np.array_equal(u, v, equal_nan=True)
    for u, v in zip(rg[0], rcg[0]):
        assert np.array_equal(u, v, equal_nan=True)
    assert not np.array_equal(rg[0][2], ra[0][2], equal_nan=True)      # and GG is not the default


@pytest.mark.parametrize('policy', ['ray-serial', 'ray-per-lane'])
def test_mixed_columns(hip_lib, policy):
    """7: 36 columns, column c with the kinds (c mod 3, (c div 3) mod 3): every column bit for bit what it is where all columns share
    its pair, also with the columns in another order"""
    name = 'rs-see21-Nra5-Nsp3-Nsp60-nco36'
    prob, block, _, _ = _case(name)
    ncol = block.ncol
    arrs = [bc.given_arrays(prob, block, c) for c in range(ncol)]
    pair = lambda c: (c % 3, (c // 3) % 3)

    def run(order, kinds_of):
        blk = ColumnBlock.concatenate([block.slice(c, c + 1) for c in order])
        e = Engine(prob, ncol, lib=hip_lib, sweep_policy=policy)
        e.set_columns(0, blk)
        for q, c in enumerate(order):
            lo, up = kinds_of(c)
            e.set_boundary(lo, up, I_lower=arrs[c][0][None] if lo == bc.GIVEN else None,
                           I_upper=arrs[c][1][None] if up == bc.GIVEN else None, col0=q, ncol=1)
        out = []
        with np.errstate(all='ignore'):
            for _ in range(2):
                e.formal_sol_gamma()
                out.append([e.get(w) for w in (I_, J_, G_)])
        st = e.boundary_state()
        e.close()
        return out, st
    ident = list(range(ncol))
    mixed, st = run(ident, pair)
    assert np.array_equal(st, np.array([pair(c) for c in ident], dtype=np.int32))
    perm = list(np.random.default_rng(7).permutation(ncol))
    mixed_p, _ = run(perm, pair)
    for q, c in enumerate(perm):
        for it in range(2):
            for u, v in zip(mixed[it], mixed_p[it]):
                assert np.array_equal(u[c], v[q], equal_nan=True), (c, q, it)
    seen = set()
    for lo in range(3):
        for up in range(3):
            shared, _ = run(ident, lambda c: (lo, up))
            for c in ident:
                if pair(c) == (lo, up):
                    seen.add(c)
                    for it in range(2):
                        for u, v in zip(mixed[it], shared[it]):
                            assert np.array_equal(u[c], v[c], equal_nan=True), (c, lo, up, it)
    assert len(seen) == ncol


@pytest.mark.parametrize('combo', ['ZZ', 'GG', 'TT'])
@pytest.mark.parametrize('name', ['rs-see13-Nra5-Nsp41-Nsp120-nco34-mul3', 'toy-see7-Nra8-Nsp21-Nsp48-nco2', 'shallow-3'])
def test_rates(hip_lib, oracle_lib, name, combo):
    """8: Engine.radiative_rates after call 1 against the reference's rates of call 2 (TT: the thermalised arm of the pass at both ends)"""
    prob, block, cols, sub = _case(name)
    ref = bc.results(name, combo, cols)
    e = Engine(prob, block.ncol, lib=hip_lib)
    e.set_columns(0, block)
    bc.set_on(e, combo, prob, block)
    with np.errstate(all='ignore'):
        e.formal_sol_gamma()
        J = e.get(J_)[cols]
        r = e.radiative_rates()
    e.close()
    runs = rt.oracle_runs(oracle_lib, prob, sub, None, None, J)       # default boundary, the same J-dagger
    for mine, w, key in ((r.Rij[cols], rt.RIJ, 'fs2_Rij'), (r.Rji_ref[cols], rt.RJI_REF, 'fs2_Rji')):
        x_def, env = runs[0][0][w], envelope.envelope(runs, 0, w)
        bound = rt.GOLDEN_BAR * np.abs(ref[key]) + rt.BASE * (np.abs(x_def) + np.abs(ref[key] - x_def)) + envelope.K_ENVELOPE * env
        ratio = float(np.max(np.abs(mine - ref[key]) / bound))
        moved = float(np.max(np.abs(ref[key] - x_def) / np.abs(x_def)))
        print('%s %s %s: %.3g x its bound (the boundary moves it by up to %.2e relative)' % (name, combo, w, ratio, moved))
        assert ratio <= 1.0, (name, combo, w, ratio)


def test_arbitrary_angle_passes_refuse_a_given_lower_boundary(hip_lib):
    """10 (the refusal): lower GIVEN raises from emergent_rays, depth_rays and emergent_spectrum with the library's message; nothing is
    launched: the context's results are bit for bit what they were"""
    prob, block = toy_problem(**ANGLES)
    e = Engine(prob, block.ncol, lib=hip_lib)
    e.set_columns(0, block)
    bc.set_on(e, 'GZ', prob, block)
    Ncont = prob.Ntrans - prob.Nlines
    lam = np.asarray(prob.wavelength)[3:9]
    spectrum = lambda: e.emergent_spectrum([1.0], lam, alpha=np.zeros((Ncont, lam.shape[0])) if Ncont else None)
    with np.errstate(all='ignore'):
        e.formal_sol_gamma()
    before = [e.get(w) for w in (I_, J_, G_, _capi.LSX_N)]
    for call in (lambda: e.emergent_rays([1.0, 0.3]), lambda: e.depth_rays([0.7]), spectrum):
        with pytest.raises(_capi.LsxError) as ei:
            call()
        assert ei.value.code == _capi.LSX_EUNSUPPORTED and 'GIVEN lower boundary' in str(ei.value), ei.value
    after = [e.get(w) for w in (I_, J_, G_, _capi.LSX_N)]
    for u, v in zip(before, after):
        assert np.array_equal(u, v, equal_nan=True)
    # one column back to a kind that is known at any angle: that column alone is served, the others still refuse
    e.set_boundary('zero', 'zero', col0=1, ncol=1)
    Iz = e.emergent_rays([1.0, 0.3], col0=1, ncol=1)
    assert np.all(np.isfinite(Iz))
    with pytest.raises(_capi.LsxError):
        e.emergent_rays([1.0, 0.3])
    e.close()


def test_lower_zero_and_thermalised_at_the_context_angles(hip_lib):
    """10 (lower Z and T at any angle), through the library alone: emergent_rays and depth_rays at the context's OWN angles give the
    up-going intensity of a formal solution with the same J-dagger -- LSX_I, and for depth_rays the start value at the deepest point:
    0 under Z, the thermalised value under T -- inside TOL = 1e-11 of the entry, the bar the project holds two implementations of one formal solution to where no exponential differs (the passes divide where the sweeps multiply by a reciprocal; the exponential is the same table)"""
    prob, block = toy_problem(**ANGLES)
    for combo in ('ZZ', 'TT'):
        e = Engine(prob, block.ncol, lib=hip_lib)
        e.set_columns(0, block)
        bc.set_on(e, combo, prob, block)
        with np.errstate(all='ignore'):
            e.formal_sol_gamma()
            J1 = e.get(J_)
            e.formal_sol_gamma()                  # J-dagger = J1
            I2 = e.get(I_)
            e.set(J_, J1)
            Ie = e.emergent_rays(prob.muz)
            d = e.depth_rays(prob.muz, what=('I',))
        e.close()
        assert np.max(np.abs(Ie - I2) / np.abs(I2)) < TOL, combo
        assert np.max(np.abs(d.I[:, :, 0, :].transpose(0, 2, 1) - I2) / np.abs(I2)) < TOL, combo
        if combo == 'ZZ':
            assert np.all(d.I[:, :, -1, :] == 0.0)
        else:
            assert np.all(d.I[:, :, -1, :] != 0.0)


def test_frozen_columns_keep_their_results(hip_lib):
    """12: a frozen column with a GIVEN boundary keeps its results bit for bit over a call; the live ones move"""
    name = 'rs-see13-Nra5-Nsp41-Nsp120-nco34-mul3'
    prob, block, _, _ = _case(name)
    e = Engine(prob, block.ncol, lib=hip_lib)
    e.set_columns(0, block)
    bc.set_on(e, 'GG', prob, block)
    with np.errstate(all='ignore'):
        e.formal_sol_gamma()
        before = [e.get(w) for w in (I_, G_)]
        mask = np.ones(block.ncol, dtype=bool)
        frozen = [0, 7, block.ncol - 1]
        mask[frozen] = False
        e.set_active_columns(mask)
        e.formal_sol_gamma()
        after = [e.get(w) for w in (I_, G_)]
    e.close()
    for u, v in zip(before, after):
        assert np.array_equal(u[frozen], v[frozen], equal_nan=True)
        assert not np.array_equal(u[mask], v[mask], equal_nan=True)


@pytest.mark.parametrize('combo', ['ZG', 'GG', 'ZT'])
def test_losses_see_both_ends(hip_lib, combo):
    """9: the Eddington flux at the top is sum_m (wmu_m / 2) mu_m (I+_m - I_upper[la][m]) (ZT: I_upper is the thermalised start value of
    the down-going rays, restated in numpy from the pass's own opacity: the thermalised arm of the losses pass at the top), I+ the emergent intensity of the same state
    -- Engine.emergent_rays at the context's angles (lower Z) or LSX_I of a call with the same J-dagger (lower G) -- to 1e-11 of the
    sum of the terms' magnitudes; and F at the top differs from the F of the same lower kind under a ZERO upper boundary by
    -4 pi sum wnu sum_m (wmu_m / 2) mu_m I_upper (the incident flux goes inwards) to the same tolerance"""
    prob, block = toy_problem(**ANGLES)
    muz, wmu = np.asarray(prob.muz), np.asarray(prob.wmu)

    def state(cb, Jdag):
        """-> (the up-going emergent intensity, the losses, J-dagger) of a context under `cb`, all three from ONE J-dagger: the J of
        the context's own first formal solution where none is handed over"""
        I_down = None
        e = Engine(prob, block.ncol, lib=hip_lib)
        e.set_columns(0, block)
        bc.set_on(e, cb, prob, block)
        with np.errstate(all='ignore'):
            if Jdag is None:
                e.formal_sol_gamma()
                Jdag = e.get(J_)
            e.set(J_, Jdag)
            e.formal_sol_gamma()
            Iup = e.get(I_)
            e.set(J_, Jdag)
            if cb[0] == 'Z':
                Irays = e.emergent_rays(muz)
                assert np.max(np.abs(Irays - Iup) / np.abs(Iup)) < TOL
                Iup = Irays
            L = e.radiative_losses(what=('F', 'H'))
            if cb[1] == 'T':           # what the down-going rays start with: the mirror image of formal_solver.py:203-207 from the pass's own opacity
                chi = e.depth_rays(muz, what=('chi',)).chi               # [ncol][nmu][Ns][nla]; ray-independent profiles: the same opacity both ways
                z, T = np.asarray(block.height), np.asarray(block.temperature)
                dtau = (1.0 / muz)[None, :, None] * (chi[:, :, 0, :] + chi[:, :, 1, :]) * 0.5 * np.abs(z[:, 0] - z[:, 1])[:, None, None]
                B0 = bc.planck(T[:, 1][:, None], np.asarray(prob.wavelength)[None, :])[:, None, :]
                B1 = bc.planck(T[:, 0][:, None], np.asarray(prob.wavelength)[None, :])[:, None, :]
                I_down = np.transpose(B1 - (B0 - B1) / dtau, (0, 2, 1))                # [ncol][Nspect][Nrays]
        e.close()
        return Iup, L, Jdag, I_down
    Iup, L, J1, I_down = state(combo, None)
    _, L0, _, _ = state(combo[0] + 'Z', J1)           # the same lower kind and J-dagger: the same up-going intensity
    I_upper = I_down if combo[1] == 'T' else np.stack([bc.given_arrays(prob, block, c)[1] for c in range(block.ncol)])
    terms = (0.5 * wmu * muz)[None, None, :] * np.stack([Iup, -I_upper])          # [2][ncol][Nspect][Nrays]
    H_top, scale = terms.sum(axis=(0, 3)), np.abs(terms).sum(axis=(0, 3))
    dev = float(np.max(np.abs(L.H[:, :, 0] - H_top) / scale))
    print('%s: H at the top, deviation %.2e of the terms\' magnitudes' % (combo, dev))
    assert dev <= 1e-11
    inc = (0.5 * wmu * muz)[None, None, :] * I_upper
    dF = -4.0 * np.pi * np.sum(L.wnu[None, :] * inc.sum(axis=2), axis=1)
    dF_scale = 4.0 * np.pi * np.sum(L.wnu[None, :] * scale, axis=1)
    devF = float(np.max(np.abs((L.F[:, 0] - L0.F[:, 0]) - dF) / dF_scale))
    print('%s: F at the top against the ZERO upper boundary, deviation %.2e' % (combo, devF))
    assert devF <= 1e-11 and np.all(np.abs(dF) > 1e-3 * np.abs(L0.F[:, 0]))


@pytest.mark.parametrize('combo', ['ZZ', 'TT', 'GG'])
def test_parabolic_mappings_agree(hip_lib, combo):
    """10 (the parabolic rule, which the reference does not have): under the new kinds its two mappings -- the ray-serial instances
    and one ray per lane -- give the same Gamma under the project's bars (off-diagonal 1e-10, diagonal 1e-11), and a Gamma that the
    boundary has moved by more than 1e-3 of its largest entry against the default"""
    name = 'rs-see13-Nra5-Nsp41-Nsp120-nco34-mul3'
    prob, block, _, _ = _case(name)

    def gamma(policy, cb):
        e = Engine(prob, block.ncol, lib=hip_lib, sweep_policy=policy)
        e.set_formal_solver('parabolic')
        e.set_columns(0, block)
        if cb is not None:
            bc.set_on(e, cb, prob, block)
        with np.errstate(all='ignore'):
            e.formal_sol_gamma()
            e.formal_sol_gamma()
        G = e.get(G_)
        e.close()
        return G
    a, b, d = gamma('ray-serial', combo), gamma('ray-per-lane', combo), gamma('ray-serial', None)
    off, diag = gamma_err(a, b, prob)
    print('parabolic %s: the two mappings differ by %.2e off the diagonal, %.2e on it' % (combo, off, diag))
    assert off < 1e-10 and diag < 1e-11
    assert np.max(np.abs(a - d)) >= 1e-3 * np.max(np.abs(d))


MUS_OFF = np.array([0.1, 0.45, 0.83])          # none of them a ray of the context


@pytest.mark.parametrize('solver', ['linear', 'parabolic'])
@pytest.mark.parametrize('combo', ['ZZ', 'TT'])
def test_arbitrary_angles_against_the_oracle_unit_entries(hip_lib, oracle_lib, combo, solver):
    """10: under lower Z and T, depth_rays at angles the context does not have gives chi, S and the up-going I at every depth; the
    oracle's unit entries piecewise_1d_impl / piecewise_parabolic_1d_impl, handed the same chi and S and the start value of the kind
    (0, or the thermalised value from chi's last two depths), give I(k) with the +-1-ulp envelope of their exponential: every entry
    inside depth_cases.BASE_I |x| + 3 |x(+1) - x(-1)|, I[kStart] included (exactly 0 under Z); emergent_rays is I[0] under the same
    bound.  This is what pins the parabolic rule's start value under the new kinds: the reference has no parabolic rule."""
    import depth_cases as dc
    prob, block = toy_problem(**ANGLES)
    e = Engine(prob, block.ncol, lib=hip_lib)
    e.set_formal_solver(solver)
    e.set_columns(0, block)
    bc.set_on(e, combo, prob, block)
    with np.errstate(all='ignore'):
        e.formal_sol_gamma()
        d = e.depth_rays(MUS_OFF, what=('chi', 'S', 'I'))
        Ie = e.emergent_rays(MUS_OFF)
    e.close()
    nmu, Ns, nla = MUS_OFF.shape[0], prob.Nspace, prob.Nspect
    mu = np.tile(MUS_OFF, nla)
    wav = np.repeat(np.asarray(prob.wavelength, dtype=np.float64), nmu)
    up = np.ones(nla * nmu, dtype=np.int32)
    planck = oracle_lib.dll.lsx_oracle_planck
    entry = oracle_lib.piecewise_1d_impl if solver == 'linear' else oracle_lib.piecewise_parabolic_1d_impl
    worst = 0.0
    for col in range(block.ncol):
        z, T = np.asarray(block.height[col], dtype=np.float64), np.asarray(block.temperature[col], dtype=np.float64)
        c2 = np.ascontiguousarray(np.transpose(d.chi[col], (2, 0, 1))).reshape(-1, Ns)          # [nla][nmu][Ns] -> rays
        S2 = np.ascontiguousarray(np.transpose(d.S[col], (2, 0, 1))).reshape(-1, Ns)
        if combo[0] == 'Z':
            Istart = np.zeros(nla * nmu)
        else:
            dtau_uw = (1.0 / mu) * (c2[:, -1] + c2[:, -2]) * 0.5 * abs(z[-1] - z[-2])           # formal_solver.py:205
            B0 = np.array([planck(float(T[-2]), float(w)) for w in wav])
            B1 = np.array([planck(float(T[-1]), float(w)) for w in wav])
            Istart = B1 - (B0 - B1) / dtau_uw
        runs = {}
        try:
            for ulp in (0, 1, -1):
                oracle_lib.dll.lsx_oracle_set_exp_ulp(int(ulp))
                runs[ulp] = entry(z, mu, up, Istart, c2, S2)[0].reshape(nla, nmu, Ns)
        finally:
            oracle_lib.dll.lsx_oracle_set_exp_ulp(0)
        mine = np.transpose(d.I[col], (2, 0, 1))                                                # [nla][nmu][Ns]
        bound = dc.BASE_I * np.abs(runs[0]) + dc.K_ENVELOPE * np.abs(runs[1] - runs[-1])
        for tag, x, x0, b in (('I(k)', mine, runs[0], bound), ('emergent', Ie[col], runs[0][:, :, 0], bound[:, :, 0])):
            dev = np.abs(x - x0)
            with np.errstate(all='ignore'):
                ratio = float(np.max(np.where(b > 0, dev / np.maximum(b, 1e-300), np.where(dev > 0, np.inf, 0.0))))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (combo, solver, col, tag, ratio)
        start = mine[:, :, -1].reshape(-1)
        if combo[0] == 'Z':
            assert np.all(start == 0.0)
        else:
            assert np.all(start != 0.0) and np.max(np.abs(start - Istart) / np.abs(Istart)) <= dc.BASE_I
    print('%s %s: I(k) and the emergent intensity at %s, %.3g x the bound at worst' % (combo, solver, MUS_OFF, worst))


def test_spectrum_under_a_zero_lower_boundary(hip_lib):
    """10 (lsx_hip_spectrum): on the context's own wavelengths, with its own background handed over, the pass is the emergent-ray pass
    -- held to it under lower ZERO inside TOL = 1e-11 of the entry (two passes of one library: the same exponential), at angles the
    context does not have; and the kind is seen: against the default boundary the spectrum moves by more than 1e-3 somewhere"""
    import final_pass_cases as fp
    prob, block = toy_problem(**ANGLES)
    blk, prof = fp.library_profiles(prob, block)
    w = np.asarray(prob.wavelength)
    alpha = np.zeros((prob.Ntrans - prob.Nlines, prob.Nspect))
    for kc, t in enumerate(t for t in prob.trans if not t.is_line):
        alpha[kc, t.Nblue:t.Nblue + t.Nlambda] = t.alpha
    out = {}
    J1 = None
    for kind in ('zero', 'thermalised'):
        e = bc.library_engine(hip_lib, prob, block, prof)
        e.set_boundary(kind, 'zero')
        with np.errstate(all='ignore'):
            if J1 is None:
                e.formal_sol_gamma()
                J1 = e.get(J_)
            e.set(J_, J1)
            out[kind] = (e.emergent_spectrum(MUS_OFF, w, alpha=alpha, bg_chi=block.bg_chi, bg_eta=block.bg_eta), e.emergent_rays(MUS_OFF))
        e.close()
    for kind, (spec, rays) in out.items():
        dev = float(np.max(np.abs(spec - rays) / np.abs(rays)))
        print('lower %s: the spectrum on the own grid against emergent_rays, %.2e relative at worst' % (kind, dev))
        assert dev <= TOL, (kind, dev)
    moved = float(np.max(np.abs(out['zero'][0] - out['thermalised'][0]) / np.abs(out['thermalised'][0])))
    print('lower zero against thermalised: the spectrum moves by up to %.2e relative' % moved)
    assert moved > 1e-3


# ---- 11: a closed isothermal cavity --------------------------------------------------------------------------------------------------
CAVITY_T = 6000.0
CAVITY_ATOMS = [(4, [('l', 0, 1, 0.500, 0.512), ('l', 0, 2, 0.300, 0.310), ('c', 1, 3, 0.00, 0.25), ('c', 2, 3, 0.05, 0.45)])]


def _cavity():
    """a made-up column in thermodynamic equilibrium at CAVITY_T: constant temperature; populations that obey Boltzmann's ratio across
    every line (the lines form a tree, so the ratios are consistent; Aji = 2hc / lambda0^3 Bji in tests/toy.py: the line source function
    is then B(T, lambda0)), n = n* (a continuum's source function is then B(T, lambda) whatever n* is); a background whose source
    function is B(T, lambda) with the scattering term sigma J-dagger at J-dagger = B; collisions in detailed balance with n*"""
    import dataclasses
    from toy import spec_problem
    prob, block = spec_problem(CAVITY_ATOMS, seed=61, Nspace=25, Nrays=5, Nspect=200, ncol=3, phi_compact=True)
    HC, KB = 6.6260755E-34 * 2.99792458E+08, 1.380658E-23
    wav = np.asarray(prob.wavelength, dtype=np.float64)
    B = bc.planck(CAVITY_T, wav)
    nst = np.array(block.nStar, dtype=np.float64)                    # [ncol][NLtot][Ns]
    lines = [t for t in prob.trans if t.is_line]
    done = {0}
    while len(done) < 1 + len(lines):                                # levels reached from the ground level along the lines' tree
        for t in lines:
            if t.i in done and t.j not in done:
                x0 = HC / (t.lambda0 * 1e-9 * KB * CAVITY_T)
                nst[:, t.j] = nst[:, t.i] * np.exp(-x0) / (t.Bji / t.Bij)         # n_i / n_j = (Bji / Bij) e^x0
                done.add(t.j)
    nst *= (np.asarray(block.nTotal)[:, 0] / nst.sum(axis=1))[:, None, :]         # one atom: the levels add up to nTotal
    nl = prob.Nlevel[0]
    C = np.array(block.C, dtype=np.float64).reshape(block.ncol, nl, nl, prob.Nspace)            # C[to][from]
    for i in range(nl):
        for j in range(i + 1, nl):
            C[:, j, i] = C[:, i, j] * nst[:, j] / nst[:, i]                       # C[j <- i] n_i = C[i <- j] n_j
    sca = np.asarray(block.bg_sca)[:, None, :]
    chi = np.asarray(block.bg_chi)
    assert np.all(chi > 2.0 * sca)
    eta = (chi - sca) * B[None, :, None]
    iso = dataclasses.replace(block, temperature=np.full_like(block.temperature, CAVITY_T), nStar=nst, n=nst.copy(),
                              C=C.reshape(block.C.shape), bg_eta=eta)
    bound = max(float(np.max(np.abs(bc.planck(CAVITY_T, wav[t.Nblue:t.Nblue + t.Nlambda]) / bc.planck(CAVITY_T, t.lambda0) - 1.0))) for t in lines)
    return prob, iso.validate(prob), B, bound


def test_closed_isothermal_cavity(hip_lib):
    """11: GIVEN I = B(T, lambda) at both ends, J-dagger = B: one formal solution gives |J / B - 1| inside the case's own
    max over lines and their wavelengths of |B(T, lambda) / B(T, lambda0) - 1| (the line source function is Planckian at line centre,
    not at lambda; computed from the grid), and a statistical equilibrium leaves |n / n* - 1| inside that bound times the LU's
    conditioning (envelope.lu_condition).  Under the default boundary the same column's J at the top is near B / 2: outside the bound,
    so the test fails without the feature"""
    from lightspinner_amd.boundary import Boundary
    prob, iso, B, bound = _cavity()
    assert 0.0 < bound < 0.3, bound
    IB = np.ascontiguousarray(np.broadcast_to(B[:, None], (prob.Nspect, prob.Nrays)))
    Jdag = np.ascontiguousarray(np.broadcast_to(B[None, :, None], (iso.ncol, prob.Nspect, prob.Nspace)))

    def run(closed):
        e = Engine(prob, iso.ncol, lib=hip_lib)
        e.set_columns(0, iso)
        if closed:
            e.set_boundary(Boundary('given', 'given', IB, IB))
        e.set(J_, Jdag)
        with np.errstate(all='ignore'):
            e.formal_sol_gamma()
            J, G = e.get(J_), e.get(G_)
            e.stat_equil()
            n = e.get(_capi.LSX_N)
        e.close()
        return J, G, n
    J, G, n = run(True)
    dev = float(np.max(np.abs(J / B[None, :, None] - 1.0)))
    cond = max(envelope.lu_condition(prob, G, iso.n, n))
    dn = float(np.max(np.abs(n / iso.nStar - 1.0)))
    Jd, _, _ = run(False)
    top = float(np.max(np.abs(Jd[:, :, 0] / B[None, :] - 1.0)))
    print('closed cavity: max |J / B - 1| = %.3e, bound %.3e; after a statistical equilibrium max |n / n* - 1| = %.3e, bound x LU '
          'conditioning %.3e (conditioning %.3g); default boundary, top: max |J / B - 1| = %.3e' % (dev, bound, dn, bound * cond, cond, top))
    assert top > bound
    assert dev <= bound
    assert dn <= bound * cond
