"""GPU side of the epilogue ledger (tests/epilogue_cases.py, tests/test_epilogue_ledger.py): every case, on 2 columns (the fused
small-batch launch with the fast-continuum kernels around it) and on 33 (one launch per tile class), against the oracle on the same
columns, and the instance the case is in the ledger for is the one that ran (lsx_hip_epilogue_info).

Bars as tests/test_toy_topologies.py, no new numbers: the first formal solution inside 1e-11 + the oracle's one-ulp-exp envelope on I and
J (tests/envelope.py), off-diagonal Gamma 1e-10, diagonal 1e-11 of its column's largest entry -- and the two Gamma entries of every
fast continuum entry by entry at 1e-10; after six iterations (statistical equilibrium from the third) the populations within 1e-8 of
the depth's largest level and J within 1e-8.  Then every third column is frozen and one more iteration runs: frozen columns keep
Gamma, n, J and I bit for bit (the kernels' colmask return), the others still meet the oracle.  The same sequence behind NaN-filled LDS
(lsx_hip_poison_lds) gives the same bits: restaged segments and cells read nothing they did not write.

Measured on an MI355X, the worst deviation of each case as a fraction of its bar (first call: I and J against 1e-11 + envelope, Gamma off-diagonal, Gamma
diagonal, continuum entries; iterated: populations, J; frozen step: populations, J), over both column counts:
  case                     I        J1     G_off    G_diag    G_cont         n         J  n_frozen  J_frozen
  r16_256               0.13    0.0049   0.00084   0.00017   0.00084   6.7e-08   1.3e-05   6.4e-08     2e-06
  r16_256_seg          0.018    0.0019    0.0007   0.00021    0.0007   1.1e-07   5.1e-07     1e-07   3.3e-06
  r16_128               0.11    0.0076   0.00019   0.00016   0.00019   2.3e-07   1.2e-05   2.2e-07   3.5e-06
  r16_128_seg           0.16     0.003   0.00026   0.00016   0.00026   1.8e-07   8.9e-06   1.5e-07   1.9e-06
  r16_64                0.14    0.0052   2.3e-05   0.00023   2.3e-05   6.2e-06   2.6e-06   3.5e-06   3.1e-06
  r16_64_seg           0.038     0.004     2e-05   0.00018     2e-05     3e-06   2.5e-06   3.1e-06   8.9e-07
  r32_256             0.0075    0.0034    0.0018   0.00026    0.0018     1e-07   5.7e-06   1.3e-07   2.4e-06
  r32_256_seg         0.0053    0.0023    0.0063   0.00069    0.0063   1.1e-07     9e-07   1.1e-07   5.5e-07
  r32_128               0.03    0.0029    0.0006   0.00014    0.0006     2e-05   6.5e-06   1.6e-05     5e-06
  r32_128_seg          0.014    0.0026    0.0017   0.00035    0.0017   1.4e-05   8.2e-06   1.9e-05   3.8e-06
  r32_64               0.014    0.0053   2.1e-05   0.00021   2.1e-05   2.8e-06   1.1e-05   2.3e-06   1.1e-05
  r32_64_seg          0.0068    0.0042     2e-05    0.0002     2e-05   3.7e-06   5.8e-06   3.2e-06   9.1e-06
  r64_256              0.011     0.011    0.0019   0.00017    0.0019   1.1e-07   5.1e-05   1.2e-07   1.3e-05
  r64_256_seg         0.0066    0.0072    0.0039   0.00086    0.0039   9.9e-08   1.3e-06   9.8e-08   1.4e-06
  r64_128             0.0033    0.0033    0.0035   0.00021    0.0035   1.5e-07     3e-06   1.3e-07   6.9e-06
  r64_128_seg         0.0047    0.0051    0.0047   0.00032    0.0047   1.7e-07   5.2e-06   1.2e-07   6.6e-07
  r64_64               0.013     0.013   1.1e-05    0.0001   1.1e-05   2.5e-06   1.4e-05   2.2e-06   1.5e-05
  r64_64_seg           0.015     0.015   2.2e-05   0.00021   2.2e-05     4e-06   3.1e-05   1.9e-06   1.3e-05
  linked1               0.11    0.0036   2.4e-05   0.00021   2.2e-05   1.3e-05   5.5e-06   8.9e-06   5.2e-06
  linked2              0.032    0.0056   8.2e-05   0.00035   3.6e-05     1e-05   4.1e-06   8.1e-06   3.2e-05
  regular5              0.15    0.0075     7e-05    0.0004     4e-05   7.2e-08     4e-06   6.6e-08   3.1e-06
  regular4              0.15    0.0035   2.4e-05   0.00021   2.2e-05   7.4e-08   2.2e-06   5.6e-08   5.5e-06
  regular4_two         0.074     0.014   2.6e-05   0.00026   2.3e-05   8.5e-08   2.5e-06   6.3e-08   7.4e-06
  regular4_two_rows    0.076    0.0054   3.4e-05   0.00022   2.5e-05   7.1e-08     2e-06   6.5e-08   1.2e-06
  simple64_64          0.018     0.023   2.8e-05   0.00027   2.8e-05   7.7e-08   4.6e-05   6.1e-08   3.6e-05
  simple64_64_seg      0.023     0.034   2.4e-05   0.00024   2.4e-05   8.1e-08     3e-05   6.8e-08   8.5e-06
  regular5:default      0.15    0.0075     7e-05   0.00038   3.9e-05   7.2e-08   3.9e-06   6.6e-08   3.1e-06
  regular4:default      0.15    0.0035   2.4e-05   0.00021   2.2e-05   6.1e-08   2.2e-06   5.6e-08   5.5e-06
  regular4_two_rows:default    0.076    0.0054   3.4e-05   0.00022   2.3e-05   7.1e-08     2e-06   6.5e-08   1.2e-06
  largest               0.16     0.034    0.0063   0.00086    0.0063     2e-05   5.1e-05   1.9e-05   3.6e-05
(I, J1: the first call, deviation over 1e-11 + 3 x the one-ulp-exp envelope, entry by entry; G_off, G_diag: gamma_err; G_cont: the
continua's own entries; n, J: after six iterations; n_frozen, J_frozen: the active columns after the step with every third column
frozen; ':default': the problem without fast_rows=1.)  With the restaging of later segments taken out of k_fast_gamma on purpose,
exactly the eighteen r*_seg parameter sets of test_case_meets_the_oracle_on_its_instance fail and every other one passes (measured
before simple64_64_seg joined the table).
"""
import ctypes as C

import numpy as np
import pytest

import envelope
from conftest import relerr, gamma_err
import epilogue_cases as ec
from lightspinner_amd import _capi
from lightspinner_amd.problem import Engine

pytestmark = pytest.mark.gpu

WHAT = dict(I=_capi.LSX_I, J=_capi.LSX_J, G=_capi.LSX_GAMMA, n=_capi.LSX_N)
PARAMS = [(name, ncol) for name in ec.CASES for ncol in ec.NCOLS]
IDS = ['%s-%d' % p for p in PARAMS]
_cache = {}


def _active(ncol):
    active = np.ones(ncol, dtype=bool)
    active[::3] = False
    return active


def _sequence(lib, prob, block, options=None, poison=None):
    """six formal solutions, statistical equilibrium from the third; then every third column frozen and one more of each.
    -> snapshots: first call, after the sixth iteration, after the frozen step; the launch counters at the last two points"""
    e = Engine(prob, block.ncol, lib=lib, options=options)
    e.set_columns(0, block)
    if lib.backend == 'oracle-c':
        lib.dll.lsx_oracle_set_threads(e._h, 8)
    out = {}
    for it in range(6):
        if poison:
            poison()
        e.formal_sol_gamma()
        if it == 0:
            out['first'] = {k: e.get(w) for k, w in WHAT.items() if k != 'n'}
        if it >= 2:
            if poison:
                poison()
            e.stat_equil()
    out['six'] = {k: e.get(w) for k, w in WHAT.items()}
    if lib.backend != 'oracle-c':
        out['info6'] = e.epilogue_info()
    e.set_active_columns(_active(block.ncol))
    if poison:
        poison()
    e.formal_sol_gamma()
    e.stat_equil()
    out['frozen'] = {k: e.get(w) for k, w in WHAT.items()}
    if lib.backend != 'oracle-c':
        out['info7'] = e.epilogue_info()
    e.close()
    return out


def _get(lib, name, ncol, key, **kw):
    """the sequence of (case, column count) on one side, computed once and shared by the tests below (never modified)"""
    k = (name, ncol, key)
    if k not in _cache:
        prob, block, options = ec.build(name, ncol)
        _cache[k] = _sequence(lib, prob, block, **kw)
    return _cache[k]


def _poison(hip_lib):
    f = hip_lib.dll.lsx_hip_poison_lds
    f.argtypes = [C.c_int32, C.c_int32]

    def run():
        assert f(0, 3) == 0
    return run


def _continuum_entries(prob, G, Gref):
    """largest relative deviation of the (i, j) and (j, i) Gamma entries of every bound-free continuum, entry by entry"""
    worst = 0.0
    for t in prob.trans:
        if t.is_line:
            continue
        nl, o = prob.Nlevel[t.atom], prob.lev2_off[t.atom]
        for a, b in ((t.i, t.j), (t.j, t.i)):
            g, r = G[:, o + a * nl + b, :], Gref[:, o + a * nl + b, :]
            assert np.all(r != 0)
            worst = max(worst, float(np.max(np.abs(g - r) / np.abs(r))))
    return worst


def _meets_the_oracle(tag, oracle_lib, prob, block, h, o):
    """the bars of the module docstring on one HIP sequence; prints and returns the fractions of the bars"""
    active = _active(block.ncol)
    # envelope.first_call_inside, keeping the fraction of the bar (1e-11 + the one-ulp-exp envelope, entry by entry) for the record
    def make():
        e = Engine(prob, block.ncol, lib=oracle_lib)
        e.set_columns(0, block)
        oracle_lib.dll.lsx_oracle_set_threads(e._h, 8)
        return e
    runs = envelope.oracle_runs(oracle_lib, make, 1, what=(_capi.LSX_I, _capi.LSX_J))
    fI = envelope.excess(h['first']['I'], runs, 0, _capi.LSX_I, 1e-11)[0]
    fJ = envelope.excess(h['first']['J'], runs, 0, _capi.LSX_J, 1e-11)[0]
    off, diag = gamma_err(h['first']['G'], o['first']['G'], prob)
    cont = _continuum_entries(prob, h['first']['G'], o['first']['G'])

    def pops(a, b):
        return float((np.abs(a - b) / np.abs(b).max(axis=1, keepdims=True)).max())
    dn, dJ = pops(h['six']['n'], o['six']['n']), relerr(h['six']['J'], o['six']['J'])
    dnf, dJf = pops(h['frozen']['n'][active], o['frozen']['n'][active]), relerr(h['frozen']['J'][active], o['frozen']['J'][active])
    frac = dict(I=fI, J1=fJ, G_off=off / 1e-10, G_diag=diag / 1e-11, G_cont=cont / 1e-10, n=dn / 1e-8, J=dJ / 1e-8, n_frozen=dnf / 1e-8, J_frozen=dJf / 1e-8)
    print('FRACTIONS %s %s' % (tag, ' '.join('%s=%.3g' % kv for kv in frac.items())))
    envelope.inside(h['first']['J'], runs, 0, _capi.LSX_J, 1e-11)
    envelope.inside(h['first']['I'], runs, 0, _capi.LSX_I, 1e-11)
    assert off < 1e-10 and diag < 1e-11, (off, diag)
    assert cont < 1e-10, cont
    assert dn < 1e-8 and dJ < 1e-8, (dn, dJ)
    assert dnf < 1e-8 and dJf < 1e-8, (dnf, dJf)
    return frac


@pytest.mark.parametrize('name,ncol', PARAMS, ids=IDS)
def test_case_meets_the_oracle_on_its_instance(hip_lib, oracle_lib, name, ncol):
    prob, block, options = ec.build(name, ncol)
    want = ec.EXPECT[name]
    h = _get(hip_lib, name, ncol, 'hip', options=options)
    o = _get(oracle_lib, name, ncol, 'oracle')
    # ---- the ledger: the expected instance ran, once per formal solution, and no other row-mapped shape
    # (2 columns: launches of their own around the fused sweep; 33: each tile class with such tiles launches its own)
    krows, kfast = (1, 1) if ncol < 32 else want['classes']
    for key, calls in (('info6', 6), ('info7', 7)):
        info = h[key]
        assert info['rows'] == {want['rows']: calls * krows}, (info, want)
        assert [c > 0 for c in info['cols']] == [c > 0 for c in want['cols']], (info, want)
        assert info['prepass'] == ((0, calls * kfast) if want['prepass_seg'] else (calls * kfast, 0)), (info, want)
        assert info['finish'] == (dict(small=calls, levels=0, lds=0) if ncol < 32 else dict(small=0, levels=calls, lds=0)), info
    print('LAUNCHED %s-%d rows=%s cols=%s prepass=%s finish=%s' % (name, ncol, h['info6']['rows'], h['info6']['cols'], h['info6']['prepass'], h['info6']['finish']))
    _meets_the_oracle('%s-%d' % (name, ncol), oracle_lib, prob, block, h, o)
    # ---- frozen columns keep their bits
    active = _active(ncol)
    for k in WHAT:
        assert np.array_equal(h['frozen'][k][~active], h['six'][k][~active]), k
    assert not np.array_equal(h['frozen']['n'][active], h['six']['n'][active])


@pytest.mark.parametrize('name,ncol', PARAMS, ids=IDS)
def test_same_bits_behind_poisoned_lds(hip_lib, name, ncol):
    """every case stages operands (SEG: again per segment) and most run the cells: NaN in every CU's LDS before each call changes nothing"""
    prob, block, options = ec.build(name, ncol)
    h = _get(hip_lib, name, ncol, 'hip', options=options)
    p = _sequence(hip_lib, prob, block, options=options, poison=_poison(hip_lib))
    for stage in ('first', 'six', 'frozen'):
        for k, v in h[stage].items():
            assert np.isfinite(p[stage][k]).all(), (stage, k)
            assert np.array_equal(p[stage][k], v), (stage, k)


@pytest.mark.parametrize('name,ncol', [p for p in PARAMS if ec.CASES[p[0]][4]], ids=[i for p, i in zip(PARAMS, IDS) if ec.CASES[p[0]][4]])
def test_row_mapped_against_column_mapped(hip_lib, oracle_lib, name, ncol):
    """the same problem without fast_rows=1: the tiles the column-mapped kernel takes by default meet the same oracle at the same bars"""
    prob, block, options = ec.build(name, ncol)
    want = ec.EXPECT[name + ':default']
    assert any(want['cols']) and options == 'fast_rows=1'
    h = _sequence(hip_lib, prob, block)
    o = _get(oracle_lib, name, ncol, 'oracle')
    info = h['info7']
    assert [c > 0 for c in info['cols']] == [c > 0 for c in want['cols']], (info, want)
    krows = 1 if ncol < 32 else want['classes'][0]
    assert info['rows'] == ({want['rows']: 7 * krows} if want['simple'] + want['cells'] else {}), (info, want)
    _meets_the_oracle('%s-%d:default' % (name, ncol), oracle_lib, prob, block, h, o)
