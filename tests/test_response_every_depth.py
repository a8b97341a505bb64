"""C5 (response_fn.py) at EVERY depth: the 2 x 82 perturbed FALC CaII columns, warm started from the reference's converged base
populations, against the reference's own converged runs (tests/golden/rf_ca_outputs.npz, make_golden.py gen_rf_outputs) --
the oracle on the CPU, the HIP library under both mappings of its sweep on the GPU.

Bars are computed, not typed in (tests/envelope.py, SequenceBars): ONE set of the oracle's three runs (exp as it is, +1 ulp,
-1 ulp) through max(niter) calls on all 164 columns, statistical equilibrium from call index 3 as drivers.iterate_mali_columns
does it, sliced per column (columns are independent, and a frozen column keeps its bits: the run without freezing holds, for
every column, what the run with the per-column stopping rule ends with -- asserted bit for bit).  A column is compared at its
own last call.  The deepest depths (k = 80, 81: the perturbed temperature enters the lower boundary condition B(T[-2:])) and
the shallowest (k = 0, 1: the emergent end point) are among them."""
import numpy as np
import pytest

import envelope

from conftest import golden, relerr, gamma_err
from lightspinner_amd import fixtures, Engine, _capi, drivers, response

NS = 82
JOBS = [(k, tag) for k in range(NS) for tag in ('p', 'm')]          # column 2k: T[k] + dT/2, column 2k + 1: T[k] - dT/2
SE_FROM = 3                                                       # test.py:20-29: the first three iterations update J only
TOL = 1e-12                                                       # the single-call bar of CaII
NEAR = 1e-6                                                       # a monitor this close to its threshold may decide one iteration either way
BOUNDARY = (0, 1, 80, 81)


def load_rf_outputs():
    """rf_ca_outputs.npz with every run's I (mu index -1) and n decoded from their bit patterns XOR the base column's"""
    d = dict(np.load(golden('rf_ca_outputs.npz')))
    bits = {'I': d['base_I'][:, -1:].copy().view(np.uint64), 'n': d['base_n'].view(np.uint64)}
    for key in list(d):
        q = key.rsplit('_', 1)[-1]
        if key[0] == 'k' and q in bits:
            d[key] = (d[key] ^ bits[q]).view(np.float64)
    return d


def test_outputs_fixture_agrees_with_the_three_depth_fixture():
    """the reference regenerates its runs deterministically: at the three depths of rf_ca.npz the new file holds the same bits"""
    new, old = load_rf_outputs(), dict(np.load(golden('rf_ca.npz')))
    for key in ('base_I', 'base_n', 'base_niter'):
        assert np.array_equal(new[key], old[key]), key
    assert sum(1 for key in new if key.endswith('_niter') and key[0] == 'k') == len(JOBS)
    for k in [int(k) for k in old['ks']]:
        for tag in ('p', 'm'):
            pre = 'k%d%s_' % (k, tag)
            assert np.array_equal(new[pre + 'I'], old[pre + 'I'][:, -1:]), pre
            assert np.array_equal(new[pre + 'n'], old[pre + 'n']), pre
            assert int(new[pre + 'niter']) == int(old[pre + 'niter']), pre
            for t in ('traj_dJ', 'traj_dPops'):
                assert np.array_equal(new[pre + t], old[pre + t], equal_nan=True), pre + t


def _near_threshold(ref, pre, dJ_tol=2e-3, dP_tol=1e-3):
    """the reference's stopping decision of this run was a near thing: a monitor within NEAR (relative) of its threshold"""
    dJ, dP = ref[pre + 'traj_dJ'], ref[pre + 'traj_dPops']
    with np.errstate(invalid='ignore'):
        return bool(np.any(np.abs(dJ / dJ_tol - 1.0) <= NEAR) or np.any(np.abs(dP[np.isfinite(dP)] / dP_tol - 1.0) <= NEAR))


class _Recorder:
    """the engine under test as drivers.iterate_mali_columns sees it, keeping what every call left behind: I, J and the per-column dJ
    after every formal solution (Gamma after the first), the populations and per-column dPops after every statistical
    equilibrium"""

    def __init__(self, eng):
        self.eng, self.ncol, self.calls = eng, eng.ncol, []

    def set_active_columns(self, mask=None):
        self.eng.set_active_columns(mask)

    def get(self, what):
        return self.eng.get(what)

    def formal_sol_gamma(self):
        dJ = self.eng.formal_sol_gamma()
        s = {w: self.eng.get(w) for w in (_capi.LSX_I, _capi.LSX_J, _capi.LSX_DJ_COL)}
        if not self.calls:
            s[_capi.LSX_GAMMA] = self.eng.get(_capi.LSX_GAMMA)
        self.calls.append(s)
        return dJ

    def stat_equil(self):
        dP = self.eng.stat_equil()
        self.calls[-1].update({w: self.eng.get(w) for w in (_capi.LSX_N, _capi.LSX_DPOPS_COL)})
        return dP


_ORACLE = {}        # one set per module: the oracle's runs and bars, shared by the oracle test and both HIP mappings


def _oracle(oracle_lib):
    if _ORACLE:
        return _ORACLE
    prob, base, raw = fixtures.load_problem_npz(golden('falc_ca.npz'))
    ref = load_rf_outputs()
    index = response.index_deltas(dict(np.load(golden('rf_ca_inputs.npz'))))
    batch = response.apply_deltas(prob, base, [(index.get(j, {}), j[0]) for j in JOBS], start_n=ref['base_n'])
    assert batch.ncol == len(JOBS)

    def make(blk):
        def f():
            e = Engine(prob, blk.ncol, lib=oracle_lib)
            e.set_columns(0, blk)
            oracle_lib.dll.lsx_oracle_set_threads(e._h, 16)
            return e
        return f
    # the oracle under the per-column stopping rule
    eng = make(batch)()
    niter = drivers.iterate_mali_columns(eng)
    I, n = eng.get(_capi.LSX_I), eng.get(_capi.LSX_N)
    eng.close()
    bars = envelope.SequenceBars(oracle_lib, make(batch), prob, int(niter.max()), SE_FROM, TOL, what=(_capi.LSX_I, _capi.LSX_GAMMA),
                                 what0=(_capi.LSX_J,))
    # the base column (I_base of the response function): its own 46 calls
    b1 = base.slice(0, 1)
    eng = make(b1)()
    niter_base = int(drivers.iterate_mali_columns(eng)[0])
    I_base, n_base = eng.get(_capi.LSX_I)[0], eng.get(_capi.LSX_N)[0]
    eng.close()
    bars_base = envelope.SequenceBars(oracle_lib, make(b1), prob, niter_base, SE_FROM, TOL, what=(_capi.LSX_I, _capi.LSX_GAMMA))
    _ORACLE.update(prob=prob, ref=ref, batch=batch, base1=b1, niter=niter, I=I, n=n, bars=bars, col=[bars.subset([c]) for c in range(len(JOBS))],
                   niter_base=niter_base, I_base=I_base, n_base=n_base, bars_base=bars_base)
    return _ORACLE


def _compared_runs(o, niter_under_test, who):
    """-> the columns whose converged state is compared with bars: every column, unless its iteration count differs from the
    reference's where the reference's stopping decision was within NEAR of a threshold (allowed +-1, printed; none expected)"""
    ref, keep, near = o['ref'], [], []
    for c, (k, tag) in enumerate(JOBS):
        pre = 'k%d%s_' % (k, tag)
        want, got = int(ref[pre + 'niter']), int(niter_under_test[c])
        if got == want:
            keep.append(c)
            continue
        assert _near_threshold(ref, pre) and abs(got - want) <= 1, ('%s: %s took %d iterations, the reference %d' % (who, pre, got, want))
        near.append(pre)
    if near:
        print('%s: iteration counts off by one where the reference stopped within %.0e of a threshold: %s' % (who, NEAR, near))
    return keep


def _oracle_vs_reference(o, c):
    """the oracle's converged column c against the reference's: (largest relative deviation of n, of I at mu index -1, the I bar, the
    ratio to the chain's cap).  n: the oracle-only bar of the column at its last call (the reference's intermediate populations are
    not in the fixture, so there is no measured deviation to feed a propagation term); I: the computed bar of its last call fed with
    the populations' measured deviation"""
    ref, b, L = o['ref'], o['col'][c], int(o['niter'][c]) - 1
    pre = 'k%d%s_' % JOBS[c]
    dn = b.check_n(o['n'][c][None], ref[pre + 'n'][None], L, ' (oracle vs reference, %s)' % pre, 0.0, quiet=True)
    bI = b.I_bar(L, dn)
    dI = relerr(o['I'][c][:, -1], ref[pre + 'I'][:, -1])
    assert dI <= bI, ('%s: I of the oracle %.3e from the reference, bar %.3e' % (pre, dI, bI))
    return dn, dI, bI, dn / b.chain_cap(L)


def _base_vs_reference(o):
    ref, b, L = o['ref'], o['bars_base'], o['niter_base'] - 1
    assert o['niter_base'] == int(ref['base_niter']) == 46
    dn = b.check_n(o['n_base'][None], ref['base_n'][None], L, ' (oracle vs reference, base column)', 0.0)
    bI = b.I_bar(L, dn)
    assert relerr(o['I_base'], ref['base_I']) <= bI
    return bI


def _rf_excess(I_p, I_m, I_b, ref_p, ref_m, ref_b, b):
    """entry by entry at mu index -1: |rf - rf_ref| against b (|I+| + |I-| + |I+ - I-|) / |I_base| (the reference's intensities), with
    b the relative bar of all three intensities: rf = (I+ - I-) / I_base moves by at most (|dI+| + |dI-|) / |I_base| +
    |I+ - I-| |dI_base| / I_base^2 (first order).  -> largest |rf - rf_ref| / bar"""
    rf = (I_p - I_m) / I_b
    rf_ref = (ref_p - ref_m) / ref_b
    bar = b * (np.abs(ref_p) + np.abs(ref_m) + np.abs(ref_p - ref_m)) / np.abs(ref_b)
    dev = np.abs(rf - rf_ref)
    return float(np.max(np.where(bar > 0, dev / np.maximum(bar, 1e-300), np.where(dev > 0, np.inf, 0.0))))


def test_response_function_every_depth_oracle_vs_reference(oracle_lib):
    """all 164 perturbed runs of the oracle against the reference's, each at its own last call: the iteration count exactly (+-1
    only where the reference's monitor lay within 1e-6 of its threshold), the per-column monitors dJ / dPops at every call (rel
    1e-6), n and I inside the computed bars of the column, and rf at every (wavelength, depth) inside
        |rf - rf_ref| <= b (|I+| + |I-| + |I+ - I-|) / |I_base|      (mu index -1)
    with b the largest of the computed I bars of the two runs and of the base column -- the bar of a difference of two nearly equal
    intensities derived from theirs (a fixed fraction of max |rf[:, k]| is too tight deep down: rf at k = 81 is 1e-6 of the
    largest)"""
    o = _oracle(oracle_lib)
    ref, bars = o['ref'], o['bars']
    # the per-column stopping rule ran every column exactly as far as the run without freezing has it at that call
    for c in range(len(JOBS)):
        L = int(o['niter'][c]) - 1
        assert np.array_equal(bars.runs[0][L][_capi.LSX_I][c], o['I'][c]) and np.array_equal(bars.runs[0][L][_capi.LSX_N][c], o['n'][c]), c
    keep = _compared_runs(o, o['niter'], 'oracle')
    # the monitors of every call against the reference's trajectories
    for c in keep:
        pre = 'k%d%s_' % JOBS[c]
        for j in range(int(o['niter'][c])):
            assert bars.runs[0][j][_capi.LSX_DJ_COL][c] == pytest.approx(ref[pre + 'traj_dJ'][j], rel=1e-6), (pre, j)
            if j >= SE_FROM:
                assert bars.runs[0][j][_capi.LSX_DPOPS_COL][c] == pytest.approx(ref[pre + 'traj_dPops'][j], rel=1e-6), (pre, j)
    bI_base = _base_vs_reference(o)
    res = {c: _oracle_vs_reference(o, c) for c in keep}
    worst = 0.0
    for k in range(NS):
        p, m = 2 * k, 2 * k + 1
        if p not in res or m not in res:
            continue
        b = max(res[p][2], res[m][2], bI_base)
        r = _rf_excess(o['I'][p][:, -1], o['I'][m][:, -1], o['I_base'][:, -1], ref['k%dp_I' % k][:, -1], ref['k%dm_I' % k][:, -1],
                       ref['base_I'][:, -1], b)
        assert r <= 1.0, ('rf at depth %d: %.2f x its derived bar' % (k, r))
        worst = max(worst, r)
    for k in BOUNDARY:
        for c in (2 * k, 2 * k + 1):
            if c in res:
                print('oracle vs reference %s: n %.2e, I %.2e (bar %.2e)' % ((('k%d%s' % JOBS[c]),) + res[c][:3]))
    print('oracle vs reference: %d runs compared with their bars; largest n %.2e, I %.2e; largest delta_n / cap %.3f; rf %.2f x its bar'
          % (len(res), max(r[0] for r in res.values()), max(r[1] for r in res.values()), max(r[3] for r in res.values()), worst))


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['ray-serial', 'ray-per-lane'])
def test_response_function_every_depth_gpu(hip_lib, oracle_lib, mode):
    """the 164 columns on HIP (ray-serial: what `auto` picks at 164 columns; ray-per-lane) under drivers.iterate_mali_columns.
    First formal solution: I and J inside the one-ulp-exp envelope of the oracle, Gamma at the single-call bars.  Every call: the
    per-column monitors against the oracle's (rel 1e-6).  Every statistical equilibrium of a column: its populations inside the
    column's computed bar, fed with its own deviation after the previous one, and below the chain's cap.  Converged, per column:
    the iteration count of the oracle and of the reference; n and I inside the computed bars against the oracle, and against the
    reference inside the sum of that bar and the oracle-vs-reference one (triangle inequality); rf inside the derived bar of
    test_response_function_every_depth_oracle_vs_reference against both"""
    o = _oracle(oracle_lib)
    prob, ref, bars, batch = o['prob'], o['ref'], o['bars'], o['batch']
    eng = Engine(prob, batch.ncol, lib=hip_lib, sweep_policy=mode)
    for a in range(0, batch.ncol, 64):
        eng.set_columns(a, batch.slice(a, min(batch.ncol, a + 64)))
    rec = _Recorder(eng)
    niter = drivers.iterate_mali_columns(rec)
    # ---- first formal solution: identical inputs
    first = rec.calls[0]
    envelope.first_call_inside(oracle_lib, prob, batch, first[_capi.LSX_I], first[_capi.LSX_J], threads=16)
    off, diag = gamma_err(first[_capi.LSX_GAMMA], bars.oracle(0, _capi.LSX_GAMMA), prob)
    assert off < 10 * TOL and diag < TOL, (off, diag)
    # ---- iteration counts
    assert np.array_equal(niter, o['niter']), np.flatnonzero(niter != o['niter'])
    keep = _compared_runs(o, niter, 'HIP %s' % mode)
    # ---- every call: monitors; every statistical equilibrium: the populations' chain, column by column
    dn_last, dn_in, ratio = np.zeros(len(JOBS)), np.zeros(len(JOBS)), 0.0
    for j, s in enumerate(rec.calls):
        live = np.flatnonzero(niter > j)
        prev = rec.calls[j - 1] if j else None
        checks = [(_capi.LSX_DJ_COL, _capi.LSX_J, prev)]
        if j >= SE_FROM:
            checks.append((_capi.LSX_DPOPS_COL, _capi.LSX_N, prev if j > SE_FROM else None))
        for w, x, p in checks:
            r = envelope.monitor_excess(s[w][live], bars.oracle(j, w)[live], s[x][live], bars.oracle(j, x)[live],
                                        None if p is None else p[x][live], None if p is None else bars.oracle(j - 1, x)[live])
            assert np.all(r <= 1.0), ('call %d: per-column monitor %s of columns %s: %s x the bar' % (j + 1, w, live[~(r <= 1.0)], r[~(r <= 1.0)]))
        if j < SE_FROM:
            continue
        for c in live:
            b = o['col'][c]
            dn_in[c] = dn_last[c]
            dn_last[c] = b.check_n(s[_capi.LSX_N][c][None], b.oracle(j, _capi.LSX_N), j, ' (HIP %s vs oracle, %s)' % (mode, 'k%d%s' % JOBS[c]),
                                   dn_in[c], quiet=True)
            ratio = max(ratio, dn_last[c] / b.chain_cap(j))
    print('check_n C5 HIP %s: largest delta_n / cap %.3f over %d statistical equilibria' % (mode, ratio, int(np.sum(np.maximum(niter - SE_FROM, 0)))))
    # ---- converged
    I, n = eng.get(_capi.LSX_I), eng.get(_capi.LSX_N)
    eng.close()
    # ---- the base column on HIP (I_base of its rf: one column, the mapping `auto` picks for it), its 46 calls against the oracle's
    bI_base_ora, bb = _base_vs_reference(o), o['bars_base']
    e0 = Engine(prob, 1, lib=hip_lib)
    e0.set_columns(0, o['base1'])
    rb = _Recorder(e0)
    nb = int(drivers.iterate_mali_columns(rb)[0])
    I_base = e0.get(_capi.LSX_I)[0]
    e0.close()
    assert nb == o['niter_base']
    dnb = dnb_in = 0.0
    for j in range(SE_FROM, nb):
        dnb_in = dnb
        dnb = bb.check_n(rb.calls[j][_capi.LSX_N], bb.oracle(j, _capi.LSX_N), j, ' (HIP vs oracle, base column)', dnb_in, quiet=True)
    print('check_n C5 HIP base column: last delta_n / cap %.3f' % (dnb / bb.chain_cap(nb - 1)))
    bI_base = bb.I_bar(nb - 1, dnb_in)
    assert relerr(I_base, o['I_base']) <= bI_base
    worst, out = 0.0, {}
    for c in keep:
        pre = 'k%d%s_' % JOBS[c]
        L, b = int(niter[c]) - 1, o['col'][c]
        bI = b.I_bar(L, dn_in[c])                              # the populations going into the last formal solution
        dI_o = relerr(I[c], o['I'][c])
        assert dI_o <= bI, ('%s: I %.3e from the oracle, bar %.3e' % (pre, dI_o, bI))
        dn_ora, _, bI_ora, _ = _oracle_vs_reference(o, c)
        bn_ora = max(b.n_bar(L, 0.0))
        dn_r, dI_r = relerr(n[c], ref[pre + 'n']), relerr(I[c][:, -1], ref[pre + 'I'][:, -1])
        assert dn_r <= max(b.n_bar(L, dn_in[c])) + bn_ora, ('%s: n %.3e from the reference' % (pre, dn_r))
        assert dI_r <= bI + bI_ora, ('%s: I %.3e from the reference, bar %.3e' % (pre, dI_r, bI + bI_ora))
        out[c] = (bI, bI_ora, dn_r, dI_r)
    for k in range(NS):
        p, m = 2 * k, 2 * k + 1
        if p not in out or m not in out:
            continue
        for who, rp, rm, rb_, b in (('oracle', o['I'][p][:, -1], o['I'][m][:, -1], o['I_base'][:, -1], max(out[p][0], out[m][0], bI_base)),
                                    ('reference', ref['k%dp_I' % k][:, -1], ref['k%dm_I' % k][:, -1], ref['base_I'][:, -1],
                                     max(out[p][0] + out[p][1], out[m][0] + out[m][1], bI_base + bI_base_ora))):
            r = _rf_excess(I[p][:, -1], I[m][:, -1], I_base[:, -1], rp, rm, rb_, b)
            assert r <= 1.0, ('rf at depth %d against the %s: %.2f x its derived bar' % (k, who, r))
            worst = max(worst, r)
    for k in BOUNDARY:
        for c in (2 * k, 2 * k + 1):
            if c in out:
                print('HIP %s vs reference k%d%s: n %.2e, I %.2e' % ((mode,) + JOBS[c] + out[c][2:]))
    print('HIP %s: %d runs compared with their bars; rf %.2f x its bar' % (mode, len(out), worst))
