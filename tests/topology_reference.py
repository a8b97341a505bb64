"""What the two sides of the reference pin on the made-up topologies share (tests/test_topologies_reference_host.py: the oracle,
tests/test_topologies_reference.py: the HIP kernels): the fixture tests/golden/topologies_*.npz (tests/golden/make_topology_golden.py:
the reference's own formal_sol_gamma_matrices / stat_equil, rh_method.py:565-745, on the golden columns of every case of
tests/topology_cases.py), the oracle's bars for the same calls, and the comparison of a run with the fixture.

The protocol: formal solutions 1-4, a statistical equilibrium behind the 3rd and the 4th.  The bars are the project's, computed from the
oracle alone (tests/envelope.py), with the FIXTURE as the centre:
  calls 1-3 (identical populations on both sides): I (and J of call 1) entry by entry inside 1e-11 |x| + 3 x what a one-ulp change of
      the oracle's exp() does to the entry; Gamma by conftest.gamma_err, off-diagonal < 1e-10, diagonal < 1e-11;
  the populations behind call 3 and 4: SequenceBars.check_n (the +-1-ulp spread, the LU's conditioning, the chain cap);
  call 4 (behind a statistical equilibrium): SequenceBars.I_bar, check_J, gamma_bar with the populations' measured deviation;
  the per-column monitors: the bar of envelope.monitor_excess; where the reference's value is not finite (the dead level: inf behind
      call 3) the same value is required.
Only the linear rule is pinned here: the reference has no parabolic rule."""
import glob
import os
import zipfile

import numpy as np

import envelope
import rates_cases as rt
import topology_cases as tc
from conftest import GOLDEN, gamma_err, relerr
from lightspinner_amd import _capi
from lightspinner_amd.problem import ColumnBlock, Engine

NCALLS, SE_FROM, TOL = 4, 2, 1e-11
I_, J_, G_, N_ = _capi.LSX_I, _capi.LSX_J, _capi.LSX_GAMMA, _capi.LSX_N
KEYS = (['fs%d_%s' % (it, k) for it in (1, 2, 3, 4) for k in ('I', 'Gamma', 'dJ')] + ['fs1_J', 'fs4_J', 'fs2_Rij', 'fs2_Rji']
        + ['se%d_%s' % (it, k) for it in (3, 4) for k in ('n', 'dPops')])

_index = {}


def fixture_index():
    """member name -> file, over tests/golden/topologies_*.npz"""
    if not _index:
        for path in sorted(glob.glob(os.path.join(GOLDEN, 'topologies_*.npz'))):
            with zipfile.ZipFile(path) as z:
                for m in z.namelist():
                    assert m.endswith('.npy') and m[:-4] not in _index, (path, m)
                    _index[m[:-4]] = path
    return _index


def _read(key):
    with np.load(fixture_index()[key]) as z:
        return z[key]


_by_digest = {}


def column_results(name, col):
    """{key: array} of the fixture for golden column `col` of case `name`; a column that an earlier case holds bit for bit is stored
    there once and found by its digest.  KeyError where the fixture has no entry."""
    idx = fixture_index()
    digest = _read('%s/c%d/digest' % (name, col))
    pre = '%s/c%d/' % (name, col)
    if pre + 'fs1_I' not in idx:
        if not _by_digest:
            for key in idx:
                if key.endswith('/fs1_I'):
                    _by_digest[_read(key[:-5] + 'digest').tobytes()] = key[:-5]
        pre = _by_digest[digest.tobytes()]
    out = {k: _read(pre + k) for k in KEYS}
    out['digest'] = digest
    return out


class Case:
    """a case of the table with the fixture's results of its golden columns, stacked over those columns"""

    def __init__(self, name):
        self.name = name
        self.prob, self.block = tc.build(name)
        self.cols = tc.golden_columns(name, self.block.ncol)
        per_col = [column_results(name, c) for c in self.cols]
        for c, r in zip(self.cols, per_col):
            assert np.array_equal(r['digest'], tc.input_digest(self.prob, self.block, c)), \
                '%s column %d: the fixture was computed from other inputs than topology_cases.build gives here' % (name, c)
        self.ref = {k: np.stack([r[k] for r in per_col]) for k in KEYS}
        self.sub = ColumnBlock.concatenate([self.block.slice(c, c + 1) for c in self.cols])

    def reference_snaps(self):
        """the fixture shaped like one run of envelope.oracle_runs (J of calls 2 and 3 is not kept)"""
        snaps = []
        for it in range(1, NCALLS + 1):
            s = {I_: self.ref['fs%d_I' % it], G_: self.ref['fs%d_Gamma' % it]}
            if 'fs%d_J' % it in self.ref:
                s[J_] = self.ref['fs%d_J' % it]
            snaps.append(s)
        return snaps


_cases, _bars = {}, {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def oracle_bars(oracle_lib, name):
    """envelope.SequenceBars of the protocol on the golden columns (computed once per case and shared)"""
    if name not in _bars:
        c = case(name)

        def make():
            e = Engine(c.prob, c.sub.ncol, lib=oracle_lib)
            e.set_columns(0, c.sub)
            oracle_lib.dll.lsx_oracle_set_threads(e._h, 8)
            return e
        with np.errstate(all='ignore'):
            _bars[name] = envelope.SequenceBars(oracle_lib, make, c.prob, NCALLS, SE_FROM, TOL)
    return _bars[name]


def run(engine, cols):
    """the protocol on a loaded engine -> per call {I, J, Gamma, dJ per column[, n, dPops per column]} of the columns `cols`"""
    snaps = []
    with np.errstate(all='ignore'):
        for it in range(NCALLS):
            engine.formal_sol_gamma()
            s = {w: engine.get(w)[cols] for w in (I_, J_, G_, _capi.LSX_DJ_COL)}
            if it >= SE_FROM:
                engine.stat_equil()
                s[N_] = engine.get(N_)[cols]
                s[_capi.LSX_DPOPS_COL] = engine.get(_capi.LSX_DPOPS_COL)[cols]
            snaps.append(s)
    return snaps


def _column_dev(a, b):
    """envelope.monitor_excess's measure: the largest relative deviation per column"""
    a, b = np.asarray(a), np.asarray(b)
    with np.errstate(all='ignore'):
        r = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
        r = np.where(np.abs(b) > 0, r, np.where(a == b, 0.0, np.inf))
    return r.reshape(r.shape[0], -1).max(axis=1)


def _monitor_ratio(m, m_ref, eps, rel=1e-6):
    """envelope.monitor_excess's bar, rel |m_ref| + 2 (1 + |m_ref|) eps, with eps given; a reference value that is not finite has to
    be met exactly.  -> the largest deviation / bar"""
    m, m_ref = np.asarray(m, dtype=np.float64), np.asarray(m_ref, dtype=np.float64)
    fin = np.isfinite(m_ref)
    assert np.array_equal(m[~fin], m_ref[~fin], equal_nan=True), (m, m_ref)
    if not fin.any():
        return 0.0
    bar = rel * np.abs(m_ref[fin]) + 2.0 * (1.0 + np.abs(m_ref[fin])) * eps[fin]
    d = np.abs(m[fin] - m_ref[fin])
    with np.errstate(all='ignore'):
        return float(np.max(np.where(bar > 0, d / np.maximum(bar, 1e-300), np.where(d > 0, np.inf, 0.0))))


def check_sequence(who, c, bars, snaps):
    """a run of the protocol (`snaps`: run()) against the fixture of case `c`.  -> {quantity: deviation / bar}, every one asserted <= 1"""
    prob, ref = c.prob, c.ref
    centre = {0: c.reference_snaps(), 1: bars.runs[1], -1: bars.runs[-1]}
    out = {}

    def put(key, ratio, detail=''):
        out[key] = max(out.get(key, 0.0), float(ratio))
        assert ratio <= 1.0, '%s, %s against the reference: %s is %.3g x its bar %s' % (c.name, who, key, ratio, detail)

    def J_bound(it):
        """what the J of two faithful implementations may differ by in a call with identical populations, per column: the single-call
        bar with the oracle's own envelope (the reference's J of calls 2 and 3 is not kept)"""
        J0 = np.abs(bars.runs[0][it][J_])
        with np.errstate(all='ignore'):
            b = TOL + envelope.K_ENVELOPE * np.where(J0 > 0, envelope.envelope(bars.runs, it, J_) / J0, 0.0)
        return b.reshape(b.shape[0], -1).max(axis=1)

    dn = 0.0
    eps_prev = np.zeros(len(c.cols))
    for it, s in enumerate(snaps):
        tag = 'fs%d_' % (it + 1)
        if it <= SE_FROM:
            r, rel, renv = envelope.excess(s[I_], centre, it, I_, TOL)
            put('I', r, '(call %d: largest deviation %.2e relative, largest envelope %.2e)' % (it + 1, rel, renv))
            if it == 0:
                r, rel, renv = envelope.excess(s[J_], centre, it, J_, TOL)
                put('J', r, '(call 1: largest deviation %.2e relative, largest envelope %.2e)' % (rel, renv))
            bo, bd = 10.0 * TOL, TOL
        else:
            put('I behind a statistical equilibrium', relerr(s[I_], ref[tag + 'I']) / bars.I_bar(it, dn), '(call %d)' % (it + 1))
            r, rel, flat = bars.J_excess(s[J_], ref[tag + 'J'], it, dn)
            put('J behind a statistical equilibrium', r, '(call %d: largest deviation %.2e relative)' % (it + 1, rel))
            bo, bd = bars.gamma_bar(it, dn, gamma_err)
        off, diag = gamma_err(s[G_], ref[tag + 'Gamma'], prob)
        put('Gamma off the diagonal', off / bo, '(call %d: %.2e)' % (it + 1, off))
        put('Gamma diagonal', diag / bd, '(call %d: %.2e)' % (it + 1, diag))
        # the monitor of J: eps measured where the fixture keeps J, the single-call bound where it does not
        eps = _column_dev(s[J_], ref[tag + 'J']) if tag + 'J' in ref else J_bound(it)
        put('dJ per column', _monitor_ratio(s[_capi.LSX_DJ_COL], ref[tag + 'dJ'], np.maximum(eps, eps_prev)), '(call %d)' % (it + 1))
        eps_prev = eps
        if it >= SE_FROM:
            n_ref = ref['se%d_n' % (it + 1)]
            n_prev, n_ref_prev = (None, None) if it == SE_FROM else (snaps[it - 1][N_], ref['se%d_n' % it])
            dev, bar = bars.n_dev(s[N_], n_ref), bars.n_bar(it, dn)
            put('n', max(d / b for d, b in zip(dev, bar)), '(behind call %d: deviation per atom %s, bars %s)' % (it + 1, dev, bar))
            dn = bars.check_n(s[N_], n_ref, it, ' (%s, %s against the reference)' % (c.name, who), dn, quiet=True)
            put('n against the chain cap', dn / bars.chain_cap(it))
            m, m_ref = s[_capi.LSX_DPOPS_COL], ref['se%d_dPops' % (it + 1)]
            fin = np.isfinite(m_ref)
            assert np.array_equal(np.asarray(m)[~fin], m_ref[~fin], equal_nan=True), (c.name, who, m, m_ref)
            if fin.any():
                sel = np.nonzero(fin)[0]
                ex = envelope.monitor_excess(np.asarray(m)[sel], m_ref[sel], s[N_][sel], n_ref[sel],
                                             None if n_prev is None else n_prev[sel], None if n_prev is None else n_ref_prev[sel])
                put('dPops per column', float(np.max(ex)), '(behind call %d: %s against %s)' % (it + 1, m, m_ref))
    return out


def oracle_rates_bars(oracle_lib, c, J):
    """rates_cases.oracle_runs on the golden columns: one call from zero on the starting populations and the given J-dagger"""
    return rt.oracle_runs(oracle_lib, c.prob, c.sub, None, None, J)


def check_rates(who, c, runs, Rij, Rji_ref):
    """the rule of tests/test_radiative_rates.py against the reference: every entry inside (oracle against the reference, asserted
    <= rates_cases.GOLDEN_BAR) |ref| + BASE |oracle| + 3 x the oracle's one-ulp-exp envelope (|ref|: the 3- and 5-depth columns have
    negative intensities at the top, the thermalised lower boundary of so thin a slab).  -> deviation / bound, the oracle's own / its bar"""
    worst, worst_o = 0.0, 0.0
    for mine, w, key in ((Rij, rt.RIJ, 'fs2_Rij'), (Rji_ref, rt.RJI_REF, 'fs2_Rji')):
        ref = c.ref[key]
        assert mine.shape == ref.shape and np.all(ref != 0)
        x0, env = runs[0][0][w], envelope.envelope(runs, 0, w)
        dref = float(np.max(np.abs(x0 - ref) / np.abs(ref)))
        assert dref <= rt.GOLDEN_BAR, '%s: the oracle\'s %s is %.2e from the reference\'s' % (c.name, w, dref)
        bound = dref * np.abs(ref) + rt.BASE * np.abs(x0) + envelope.K_ENVELOPE * env
        ratio = float(np.max(np.abs(mine - ref) / bound))
        assert ratio <= 1.0, '%s, %s: %s is %.3g x its bound against the reference' % (c.name, who, w, ratio)
        worst, worst_o = max(worst, ratio), max(worst_o, dref / rt.GOLDEN_BAR)
    return worst, worst_o
