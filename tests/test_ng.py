"""Ng acceleration of the MALI loop on the GPU (include/lsx_hip_ng.h; Engine.configure_ng / ng_state, Context(ng=...)).

The checker is tests/ng_cases.py: exact arithmetic (mpmath) on read-back histories for the extrapolation itself, the numpy
restatement of the scheme over the oracle (pinned in tests/test_ng_host.py) for whole runs."""
import numpy as np
import pytest

import ng_cases as ng
from conftest import golden
from helpers import build_fakes
from lightspinner_amd import _capi, drivers, synth
from lightspinner_amd.problem import Engine, NgOptions
from lightspinner_amd.rh_method import Context
from toy import spec_problem

pytestmark = pytest.mark.gpu
U = ng.U
N, DP = _capi.LSX_N, _capi.LSX_DPOPS_COL


def shape_case(shape):
    """-> (prob, one-column block)"""
    if shape == 'tiny':
        # three depths, one two-level atom with one line: 6 elements for 256 threads.  Made up, and collision dominated (the rates
        # times 1000) so that its populations stay positive and settle slowly enough for a history that moves
        prob, block = spec_problem([(2, [('l', 0, 1, .3, .7)])], seed=3, Nspace=3, Nrays=3, Nspect=40, ncol=1, phi_compact=True)
        block.C *= 1e3
        return prob, block
    if shape == 'ca325':
        import rates_cases
        return rates_cases.refined('falc_ca.npz', ncol=1)         # 6 x 325 = 1950 elements: eight passes of the block
    prob, block, _ = ng.problem(shape)
    return prob, block


def pair(hip_lib, prob, block, ncol=1):
    a, b = Engine(prob, ncol, lib=hip_lib), Engine(prob, ncol, lib=hip_lib)
    a.set_columns(0, block)
    b.set_columns(0, block)
    return a, b


def iteration(e):
    e.formal_sol_gamma()
    return e.stat_equil()


# ---- 1. the extrapolation itself -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('delay', [0, 2])
@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('shape', ['tiny', 'ca', 'cah', 'ca325'])
def test_the_extrapolation_itself(hip_lib, shape, order, delay):
    """engine A plain, engine B with Ng: bit-equal up to the statistical equilibrium before the step; at the step B's coefficients
    against the exact solve of the exact sums of A's read-back history within ng_cases.coefficients_bar (K = 4), B's populations
    against the combination with B's own coefficients within (order + 3) u (...), B's monitor against numpy's from B's populations"""
    prob, block = shape_case(shape)
    A, B = pair(hip_lib, prob, block)
    B.configure_ng(order, delay)
    for _ in range(ng.N_LAMBDA_ONLY):
        assert A.formal_sol_gamma() == B.formal_sol_gamma()
    hist, last = [], delay + order + 1
    for k in range(last + 1):
        dPa, dPb = iteration(A), iteration(B)
        nA, nB, st = A.get(N)[0], B.get(N)[0], B.ng_state()
        if k >= delay:
            hist.insert(0, nA)
        if k < last:                                    # Ng only stores
            assert np.array_equal(nA, nB) and dPa == dPb
            assert (st.stored[0], st.applied[0], st.rejected[0]) == (k + 1 - delay, 0, 0) and not st.coef.any()
    assert (st.stored[0], st.applied[0], st.rejected[0]) == (0, 1, 0)
    assert not np.array_equal(nA, nB)
    assert len(hist) == order + 2 and all(np.all(h > 0) for h in hist)
    for a in range(prob.Natoms):
        sl = slice(prob.lev_off[a], prob.lev_off[a] + prob.Nlevel[a])
        xs = [h[sl] for h in hist]
        c_dev = st.coef[0, a, :order]
        c, cond = ng.exact_coefficients(xs, order)
        bar, rel = ng.coefficients_bar(xs[0].size, order, cond, c)
        err = float(np.max(np.abs(c_dev - c)))
        print('%s order %d delay %d atom %d: c = %s, cond(A) = %.2e, |c_dev - c| = %.2e, %.3f x the bar (relative bound %.1e)'
              % (shape, order, delay, a, c, cond, err, err / bar, rel))
        assert rel <= 1e-6, 'vacuous: cond(A) = %.2e' % cond
        assert err <= bar
        if order == 1:
            assert st.coef[0, a, 1] == 0.0
        r = ng.combination_excess(nB[sl], c_dev, xs)
        print('    populations against the combination with the device coefficients: %.3f x the bar' % r)
        assert r <= 1.0
    assert np.all(np.isfinite(nB)) and np.all(nB > 0)
    want = float(np.max(np.abs(1.0 - hist[1] / nB)))
    got = float(B.get(DP)[0])
    assert got == dPb                                   # one column: lsx_stat_equil's value is the column's
    assert abs(got - want) <= 4 * U * (1.0 + float(np.max(np.abs(hist[1] / nB))))
    A.close()
    B.close()


# ---- 2. placement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', [1, 2])
def test_a_column_has_the_same_bits_wherever_it_sits(hip_lib, order):
    prob, block, raw = ng.problem('ca')
    batch, _ = synth.perturbed_columns(prob, block, raw, ncol=7, seed=1234, vlos_sigma=0.0)
    big = Engine(prob, 7, lib=hip_lib)
    big.set_columns(0, batch)
    big.configure_ng(order)
    nit = 2 * (order + 2)                               # through two steps
    for _ in range(ng.N_LAMBDA_ONLY):
        big.formal_sol_gamma()
    for _ in range(nit):
        iteration(big)
    nb, dpb, sb = big.get(N), big.get(DP), big.ng_state()
    assert np.all(sb.applied == 2) and np.all(sb.stored == 0) and np.all(sb.rejected == 0)
    for c in (0, 3, 6):
        one = Engine(prob, 1, lib=hip_lib)
        one.set_columns(0, batch.slice(c, c + 1))
        one.configure_ng(order)
        for _ in range(ng.N_LAMBDA_ONLY):
            one.formal_sol_gamma()
        for _ in range(nit):
            iteration(one)
        so = one.ng_state()
        assert np.array_equal(one.get(N)[0], nb[c]) and one.get(DP)[0] == dpb[c]
        assert np.array_equal(so.coef[0], sb.coef[c]) and so.coef[0, :, :order].all()
        assert (so.stored[0], so.applied[0], so.rejected[0]) == (sb.stored[c], sb.applied[c], sb.rejected[c])
        one.close()
    big.close()


# ---- 3. the state machine -------------------------------------------------------------------------------------------------
def three_columns(hip_lib, order, delay=0):
    prob, block, raw = ng.problem('ca')
    batch, _ = synth.perturbed_columns(prob, block, raw, ncol=3, seed=77, vlos_sigma=0.0)
    e = Engine(prob, 3, lib=hip_lib)
    e.set_columns(0, batch)
    e.configure_ng(order, delay)
    for _ in range(ng.N_LAMBDA_ONLY):
        e.formal_sol_gamma()
    return prob, batch, e


def test_a_frozen_column_keeps_its_history_and_resumes(hip_lib):
    prob, batch, e = three_columns(hip_lib, 1)
    iteration(e)
    assert e.ng_state().stored.tolist() == [1, 1, 1]
    n1 = e.get(N)[1]
    e.set_active_columns([True, False, True])
    iteration(e)
    assert e.ng_state().stored.tolist() == [2, 1, 2] and np.array_equal(e.get(N)[1], n1)
    iteration(e)
    st = e.ng_state()
    assert st.stored.tolist() == [0, 1, 0] and st.applied.tolist() == [1, 0, 1] and np.array_equal(e.get(N)[1], n1)
    e.set_active_columns(None)
    iteration(e)
    assert e.ng_state().stored.tolist() == [1, 2, 1]
    iteration(e)
    st = e.ng_state()
    assert st.stored.tolist() == [2, 0, 2] and st.applied.tolist() == [1, 1, 1] and st.rejected.tolist() == [0, 0, 0]
    assert st.coef[1, 0, 0] != 0.0
    e.close()


def test_new_populations_reset_their_columns_only(hip_lib):
    prob, batch, e = three_columns(hip_lib, 2, delay=1)
    assert e.ng_state().stored.tolist() == [-1, -1, -1]
    for _ in range(3):
        iteration(e)
    assert e.ng_state().stored.tolist() == [2, 2, 2]
    e.set(N, e.get(N, 1, 1), col0=1)                    # lsx_set(LSX_N) on column 1
    assert e.ng_state().stored.tolist() == [2, -1, 2]
    iteration(e)
    assert e.ng_state().stored.tolist() == [3, 0, 3]
    e.set_columns(2, batch.slice(2, 3))                 # lsx_set_columns on column 2
    st = e.ng_state()
    assert st.stored.tolist() == [3, 0, -1] and not st.applied.any() and not st.rejected.any()
    e.set(_capi.LSX_J, e.get(_capi.LSX_J, 0, 1), col0=0)      # J is not the populations
    assert e.ng_state().stored.tolist() == [3, 0, -1]
    e.configure_ng(2, 1)                                # configuring resets every column
    assert e.ng_state().stored.tolist() == [-1, -1, -1]
    e.close()


def test_switching_it_off_restores_the_plain_engine_bit_for_bit(hip_lib):
    prob, block, _ = ng.problem('ca')
    A, B = pair(hip_lib, prob, block)
    plain = B.effective_options(), B.options_signature()
    assert plain == (A.effective_options(), A.options_signature()) and ';ng=' not in plain[0]
    B.configure_ng(2, 1)
    assert B.effective_options() == plain[0] + ';ng=2,1' and B.options_signature() != plain[1]
    for _ in range(ng.N_LAMBDA_ONLY):
        A.formal_sol_gamma()
        B.formal_sol_gamma()
    for _ in range(2):                                  # the delay and one stored vector: B's populations are still A's
        iteration(A)
        iteration(B)
    B.configure_ng(0)
    assert (B.effective_options(), B.options_signature()) == plain
    with pytest.raises(_capi.LsxError):
        B.ng_state()
    for _ in range(3):
        assert A.formal_sol_gamma() == B.formal_sol_gamma() and A.stat_equil() == B.stat_equil()
        for what in (N, _capi.LSX_J, _capi.LSX_I, _capi.LSX_GAMMA):
            assert np.array_equal(A.get(what), B.get(what))
    A.close()
    B.close()


def test_bad_orders_and_delays_are_refused(hip_lib):
    prob, block, _ = ng.problem('ca')
    e = Engine(prob, 1, lib=hip_lib)
    for order, delay in ((3, 0), (-1, 0), (7, 0), (2, -1), (1, -5)):
        with pytest.raises(_capi.LsxError) as ei:
            e.configure_ng(order, delay)
        assert ei.value.code == _capi.LSX_EINVAL
        assert ';ng=' not in e.effective_options()
    e.configure_ng(1)
    with pytest.raises(_capi.LsxError):
        e.ng_state(1, 1)                                # a column range outside the context
    e.close()


def overshooting_start(prob, n):
    """populations handed in so that a later extrapolation overshoots: the ground level of the upper half of the atmosphere
    divided by e^3.  Found on the CPU (the restatement over the oracle): every statistical equilibrium that follows gives positive
    populations, the first two steps of order 2 are taken, the third would put 47 entries at or below zero (down to -0.94 x0)."""
    f = np.ones_like(n)
    f[:, 0, :prob.Nspace // 2] = np.exp(-3.0)
    return n * f


def test_a_step_that_would_go_non_positive_is_rejected(hip_lib, oracle_lib):
    prob, block, _ = ng.problem('ca')
    # what the restatement does on the oracle
    o = Engine(prob, 1, lib=oracle_lib)
    o.set_columns(0, block)
    for _ in range(ng.N_LAMBDA_ONLY):
        o.formal_sol_gamma()
    o.set(N, overshooting_start(prob, o.get(N)))
    col, expect = ng.NgColumn(prob, 2), []
    for k in range(12):
        iteration(o)
        step = col.after_stat_equil(o.get(N)[0])
        if step is not None:
            o.set(N, step[0][None])
        expect.append((col.stored, col.applied, col.rejected))
    assert expect[-1] == (0, 2, 1) and expect[-2] == (3, 2, 0)
    o.close()
    # B accelerates itself; A, without Ng, is handed B's populations and J before every iteration: A's result is what the
    # statistical equilibrium wrote in B
    A, B = pair(hip_lib, prob, block)
    B.configure_ng(2)
    for _ in range(ng.N_LAMBDA_ONLY):
        B.formal_sol_gamma()
    B.set(N, overshooting_start(prob, B.get(N)))
    assert B.ng_state().stored[0] == 0
    for k in range(12):
        A.set(N, B.get(N))
        A.set(_capi.LSX_J, B.get(_capi.LSX_J))
        dPa, dPb = iteration(A), iteration(B)
        st = B.ng_state()
        assert (st.stored[0], st.applied[0], st.rejected[0]) == expect[k], k
        same = np.array_equal(A.get(N), B.get(N))
        took = k > 0 and expect[k][1] > expect[k - 1][1]
        assert same != took, k                          # bit-equal to the solve's result unless a step was taken
        if not took:
            assert dPa == dPb
    assert np.all(B.get(N) > 0)
    A.close()
    B.close()


# ---- 4. end to end --------------------------------------------------------------------------------------------------------
_GPU_RUNS = {}


def gpu_plain(hip_lib, case, tight):
    if (case, tight) not in _GPU_RUNS:
        prob, block, _ = ng.problem(case)
        e = Engine(prob, 1, lib=hip_lib)
        e.set_columns(0, block)
        _GPU_RUNS[case, tight] = ng.iterate(e, **(dict(dJ_tol=1e-8, dPops_tol=1e-8) if tight else {}))
        e.close()
    return _GPU_RUNS[case, tight]


@pytest.mark.parametrize('case', ['ca', 'cah'])
def test_convergence_through_engine_and_context(hip_lib, oracle_lib, case):
    prob, block, raw = ng.problem(case)
    want = ng.oracle_run(oracle_lib, case, 2)
    e = Engine(prob, 1, lib=hip_lib)
    e.set_columns(0, block)
    e.configure_ng(NgOptions(2))
    r = ng.iterate(e)
    st = e.ng_state()
    print('%s: %d iterations with Ng of order 2 (restatement over the oracle: %d), %d steps, %d rejected'
          % (case, r.n_iter, want.n_iter, st.applied[0], st.rejected[0]))
    assert r.converged and r.n_iter == want.n_iter == ng.NG_ITERATIONS[case, 2]
    assert (st.applied[0], st.rejected[0]) == (want.applied, 0)
    assert np.allclose(r.dJ, want.dJ, rtol=1e-6)
    assert np.allclose(r.dPops[3:], want.dPops[3:], rtol=1e-6)
    plain_count = len(raw['traj_dJ']) if len(raw['traj_dJ']) > 8 else ng.PLAIN_ITERATIONS[case]     # (falc_cah.npz records 8 only)
    assert plain_count == ng.PLAIN_ITERATIONS[case]
    plain, tight = gpu_plain(hip_lib, case, False), gpu_plain(hip_lib, case, True)
    assert r.n_iter < plain_count and plain.n_iter == plain_count
    d_ng, d_plain = ng.popdist(r.n, tight.n), ng.popdist(plain.n, tight.n)
    print('%s: off the plain 1e-8 run (%d iterations) by %.2e with Ng, %.2e plain' % (case, tight.n_iter, d_ng, d_plain))
    assert tight.converged and d_ng <= d_plain
    # the pipelined engine loop: the same iterations, the same bits
    e.set_columns(0, block)                             # (resets the history)
    h = drivers.iterate_mali_engine(e)
    assert h.converged and h.dJ == r.dJ and h.dPops[3:] == r.dPops[3:] and np.array_equal(e.get(N)[0], r.n)
    e.close()
    # Context(ng=...): the drop-in boundary, with its speculative formal solution behind every stat_equil.  It builds its line
    # profiles on the device, so its inputs differ from the fixture's arrays in the last bits: against the restatement it is held
    # like the engine above, and bit for bit against the plain Engine calls on the columns of a second, identical Context
    ctx = Context(*build_fakes(dict(raw)), lib=hip_lib, ng=NgOptions(2))
    assert ctx._engine.effective_options().endswith(';ng=2,0')
    hc = drivers.iterate_mali(ctx)
    assert hc.converged and hc.n_iter == want.n_iter
    assert np.allclose(hc.dJ, want.dJ, rtol=1e-6) and np.allclose(hc.dPops[3:], want.dPops[3:], rtol=1e-6)
    twin = Context(*build_fakes(dict(raw)), lib=hip_lib, ng=NgOptions(2))
    rt = ng.iterate(twin._engine)
    assert hc.dJ == rt.dJ and hc.dPops[3:] == rt.dPops[3:]
    assert np.array_equal(np.concatenate([a.n for a in ctx.activeAtoms]), rt.n)
    sc, stw = ctx._engine.ng_state(), twin._engine.ng_state()
    assert np.array_equal(sc.coef, stw.coef) and (sc.applied[0], sc.rejected[0]) == (stw.applied[0], stw.rejected[0]) == (want.applied, 0)
    ctx.close()
    twin.close()


def test_columns_with_their_own_stopping_rule(hip_lib):
    """iterate_mali_columns on seven perturbed columns with Ng on: every column's count and populations are those of the column
    run alone"""
    prob, block, raw = ng.problem('ca')
    batch, _ = synth.perturbed_columns(prob, block, raw, ncol=7, seed=4321, vlos_sigma=0.0)
    big = Engine(prob, 7, lib=hip_lib)
    big.set_columns(0, batch)
    big.configure_ng(2)
    n_iter = drivers.iterate_mali_columns(big)
    nb, sb = big.get(N), big.ng_state()
    print('iterations per column with Ng of order 2: %s, steps %s' % (n_iter.tolist(), sb.applied.tolist()))
    assert not sb.rejected.any() and np.all(n_iter < ng.PLAIN_ITERATIONS['ca'] + 10)
    for c in range(7):
        one = Engine(prob, 1, lib=hip_lib)
        one.set_columns(0, batch.slice(c, c + 1))
        one.configure_ng(2)
        assert drivers.iterate_mali_columns(one).tolist() == [n_iter[c]]
        assert np.array_equal(one.get(N)[0], nb[c])
        so = one.ng_state()
        assert (so.stored[0], so.applied[0]) == (sb.stored[c], sb.applied[c]) and np.array_equal(so.coef[0], sb.coef[c])
        one.close()
    big.close()


def test_the_response_function_takes_the_option(hip_lib):
    """run_response_function(ng=...) on the three recorded depths: the base engine and the batch both accelerate"""
    from lightspinner_amd import response
    prob, base, raw = ng.problem('ca')
    rf = dict(np.load(golden('rf_ca.npz')))
    ks = [int(k) for k in rf['ks']]
    plain_counts = np.array([int(rf['k%d%s_niter' % (k, tag)]) for k in ks for tag in ('p', 'm')])
    out = response.run_response_function(prob, base, rf, ks, lib=hip_lib, ng=NgOptions(2))
    print('response function with Ng of order 2: base %d iterations, perturbed columns %s (plain: %s)'
          % (out['n_iter_base'], np.asarray(out['n_iter']).tolist(), plain_counts.tolist()))
    assert out['n_iter_base'] == ng.NG_ITERATIONS['ca', 2]
    assert np.all(np.isfinite(out['rf'])) and out['rf'].shape == (prob.Nspect, len(ks))
    assert np.all(np.asarray(out['n_iter']) >= ng.N_LAMBDA_ONLY + 1)
