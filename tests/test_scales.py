"""Depth-scale conversion on the device (include/lsx_hip_scales.h): lsx_hip_convert_scales against the UNMODIFIED reference's
AtmosphereConstructor.convert_scales (tests/golden/scales_falc.npz) inside the bar of tests/scales_cases.py; every depth count and
the chunk boundaries of the kernel's LDS staging; placement bit for bit; outputs left out; the install path; the errors.

The kernel stages SC_KC = 16 depths at a time (lightspinner_amd/csrc/lsx_background.hip): the 33-, 40-, 82- and 325-depth columns
cross a chunk boundary (33 = 2 x 16 + 1 ends one depth into a chunk), the 2-, 3-, 4- and 12-depth ones end inside the first.

Measured on MI355X (fraction of the bound, worst entry): see DESIGN.md 2, "The depth scales: how they are pinned"."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import scales_cases as sc
from conftest import golden
from lightspinner_amd import ColumnBlock, Engine, _capi, fixtures
from lightspinner_amd import atmosphere as lsa
from lightspinner_amd.background import _carrier_problem

pytestmark = pytest.mark.gpu

SC_KC = 16


@pytest.fixture(scope='module')
def carriers(hip_lib):
    """one carrier engine per depth count, made on first use"""
    made = {}

    def get(Nspace):
        if Nspace not in made:
            made[Nspace] = Engine(_carrier_problem(Nspace), 1, lib=hip_lib)
        return made[Nspace]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope='module')
def falc():
    return fixtures.load_problem_npz(golden('falc_ca.npz'))


@pytest.fixture(scope='module')
def host():
    return sc.HostLib()


def convert(eng, case, **kw):
    return eng.convert_scales(sc.tables(), case.scale, case.ds, case.T, case.nH, case.ne, logG=float(sc.fixture()['logG']), **kw)


def columns(scale, n):
    """n columns of 82 depths on one scale, cycling through FALC and its six perturbed versions -> ds, T, nH, ne [n][82]"""
    suffix = {sc.GEO: '_geo', sc.CM: '_cm', sc.TAU: '_tau'}[scale]
    src = [sc.Case(p + suffix) for p in ('falc', 'p0', 'p1', 'p2', 'p3', 'p4', 'p5')]
    pick = [src[i % 7] for i in range(n)]
    return tuple(np.array([getattr(c, k) for c in pick]) for k in ('ds', 'T', 'nH', 'ne'))


def same(a, b):
    for q in ('height', 'cmass', 'tau_ref', 'chi_ref'):
        assert np.array_equal(getattr(a, q), getattr(b, q)), q


# ---- 1. every case of the fixture against the reference -------------------------------------------------------------------------
@pytest.mark.parametrize('name', sc.cases())
def test_case_against_the_reference(carriers, name):
    c = sc.Case(name)
    r = convert(carriers(c.N), c)
    sc.check_case(c, r.height[0], r.cmass[0], r.tau_ref[0], r.chi_ref[0])


class StandIn:
    """a Lightspinner-shaped constructor: the attributes atmosphere.convert_scales reads, and the two methods it calls"""

    class Scale:
        def __init__(self, name):
            self.name = name

    def __init__(self, case):
        self.depthScale, self.temperature, self.nHTot, self.ne = case.ds.copy(), case.T.copy(), case.nH.copy(), case.ne.copy()
        self.scale = StandIn.Scale({sc.GEO: 'Geometric', sc.CM: 'ColumnMass', sc.TAU: 'Tau500'}[case.scale])
        self.calls = []

    def nondimensionalise(self):
        self.calls.append('nd')

    def dimensionalise(self):
        self.calls.append('d')


@pytest.mark.parametrize('name', ['falc_cm', 'falc_geo', 'falc_tau'])
def test_drop_in_on_a_constructor(name):
    c = sc.Case(name)
    a = StandIn(c)
    assert lsa.convert_scales(a, sc.tables(), logG=float(sc.fixture()['logG'])) is a
    assert a.calls == ['nd', 'd']
    assert a.height.shape == a.cmass.shape == a.tau_ref.shape == (82,)
    sc.check_case(c, a.height, a.cmass, a.tau_ref, None, tag='drop-in: ')


# ---- 2. depth counts: the integration on the device is the host's, bit for bit, given the device's own opacity ------------------
@pytest.mark.parametrize('N', [2, 3, 4, 33, 40, 82, 325])
def test_depth_counts_and_chunk_boundaries(carriers, host, N):
    """Only + - * / follow the opacity, and the unit is built without contraction: fed the chi_ref the device returns, the CPU build of
    the same header must give the device's height, cmass and tau_ref bit for bit (that build is pinned against the reference, given
    the reference's opacity, in tests/test_scales_host.py).  Slices of the 325-depth column, which cross 0 .. 20 chunk boundaries."""
    assert sum(n > SC_KC and n % SC_KC != 0 for n in (33, 40, 82, 325)) >= 2
    fine = sc.Case('fine_cm')
    lo = {2: 300, 3: 150, 4: 321}.get(N, 0)
    s = slice(lo, lo + N)
    T, nH = fine.T[s], fine.nH[s]
    ne = 1e-4 * nH
    eng, tab, g = carriers(N), sc.tables(), sc.gravity()
    base = eng.convert_scales(tab, 'column_mass', fine.ds[s], T, nH)
    for scale, ds in ((sc.CM, fine.ds[s]), (sc.GEO, base.height[0]), (sc.TAU, base.tau_ref[0])):
        r = eng.convert_scales(tab, scale, ds, T, nH, ne)
        assert np.array_equal(r.chi_ref, base.chi_ref)
        rc, h, cm, tau = host.integrate(scale, tab.weight_per_H, ds, T, nH, ne, g, r.chi_ref[0])
        assert rc == 0, host.error()
        assert np.array_equal(r.height, h) and np.array_equal(r.cmass, cm) and np.array_equal(r.tau_ref, tau), (N, scale)
        assert np.all(np.diff(r.tau_ref[0]) > 0) and np.all(np.diff(r.height[0]) < 0) and np.all(np.diff(r.cmass[0]) > 0)
        if scale == sc.GEO:
            assert np.array_equal(r.height[0], ds)


# ---- 3. placement, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', [sc.CM, sc.GEO, sc.TAU])
def test_placement_bit_for_bit(carriers, scale):
    eng, tab = carriers(82), sc.tables()
    one = sc.Case('p3' + {sc.GEO: '_geo', sc.CM: '_cm', sc.TAU: '_tau'}[scale])
    alone = convert(eng, one)
    for pos in (0, 31, 63, 64):
        ds, T, nH, ne = columns(scale, 65)
        ds[pos], T[pos], nH[pos], ne[pos] = one.ds, one.T, one.nH, one.ne
        r = eng.convert_scales(tab, scale, ds, T, nH, ne)
        for q in ('height', 'cmass', 'tau_ref', 'chi_ref'):
            assert np.array_equal(getattr(r, q)[pos], getattr(alone, q)[0]), (pos, q)
    ds, T, nH, ne = columns(scale, 130)
    whole = eng.convert_scales(tab, scale, ds, T, nH, ne)
    for half in (slice(0, 65), slice(65, 130)):
        part = eng.convert_scales(tab, scale, ds[half], T[half], nH[half], ne[half])
        for q in ('height', 'cmass', 'tau_ref', 'chi_ref'):
            assert np.array_equal(getattr(whole, q)[half], getattr(part, q)), q
    assert not np.array_equal(whole.tau_ref[0], whole.tau_ref[1])


# ---- 4. outputs left NULL ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', [sc.CM, sc.GEO, sc.TAU])
def test_outputs_left_out_do_not_change_the_others(carriers, scale):
    eng, tab = carriers(82), sc.tables()
    ds, T, nH, ne = (_capi.f64(a) for a in columns(scale, 3))
    full = eng.convert_scales(tab, scale, ds, T, nH, ne)
    ctab, _keep = tab.to_c()
    names = ('height', 'cmass', 'tau_ref', 'chi_ref')
    for mask in range(16):
        out = [np.full((3, 82), np.nan) if mask >> i & 1 else None for i in range(4)]
        rc = eng.lib.dll.lsx_hip_convert_scales(eng._h, C.byref(ctab), scale, 0, 3, _capi._ptr(ds), _capi._ptr(T), _capi._ptr(nH), _capi._ptr(ne),
                                                sc.gravity(), *[None if a is None else _capi._ptr(a) for a in out], 0)
        assert rc == 0, mask
        for a, q in zip(out, names):
            if a is not None:
                assert np.array_equal(a, getattr(full, q)), (mask, q)
    if scale != sc.GEO:         # ne is not read: NULL is as good as an array
        r = eng.convert_scales(tab, scale, ds, T, nH, None)
        same(r, full)


# ---- 5. install --------------------------------------------------------------------------------------------------------------------
def _three(prob, block):
    return ColumnBlock.concatenate([block, block, block]).validate(prob)


def _one_fs(eng):
    return [eng.formal_sol_gamma()] + [eng.get(w) for w in (_capi.LSX_I, _capi.LSX_J, _capi.LSX_GAMMA)]


def _equal(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize('policy,scale', [('ray-per-lane', sc.CM), ('ray-serial', sc.CM), ('ray-serial', sc.TAU), ('ray-per-lane', sc.GEO)])
def test_install_equals_set_columns_with_the_returned_heights(hip_lib, falc, policy, scale):
    prob, block, _ = falc
    cols = _three(prob, block)
    ds, T, nH, ne = columns(scale, 4)
    ds, T, nH, ne = ds[1:], T[1:], nH[1:], ne[1:]           # p0, p1, p2
    tab = sc.tables()
    A, B = (Engine(prob, 3, lib=hip_lib, sweep_policy=policy) for _ in range(2))
    r = A.convert_scales(tab, scale, ds, T, nH, ne)
    assert not np.array_equal(r.height[0], r.height[1]) and not np.array_equal(r.height[0], cols.height[0])
    A.set_columns(0, dataclasses.replace(cols, height=r.height))
    wrong = dataclasses.replace(cols, height=1.25 * cols.height)
    B.set_columns(0, wrong)
    r2 = B.convert_scales(tab, scale, ds, T, nH, ne, install=True)
    same(r, r2)
    a, b = _one_fs(A), _one_fs(B)
    _equal(a, b)
    # ... and the wrong heights would have shown; an install behind a formal solution is seen by the next one (the ray-serial
    # sweeps' operand table is rebuilt); without read-back nothing comes back
    W = Engine(prob, 3, lib=hip_lib, sweep_policy=policy)
    W.set_columns(0, wrong)
    w = _one_fs(W)
    assert not np.array_equal(w[1], a[1])
    assert W.convert_scales(tab, scale, ds, T, nH, ne, install=True, read_back=False) is None
    A.close(); B.close(); W.close()


def test_install_into_a_sub_range(hip_lib, falc):
    prob, block, _ = falc
    cols = _three(prob, block)
    ds, T, nH, ne = columns(sc.CM, 3)
    tab = sc.tables()
    A, B = Engine(prob, 3, lib=hip_lib), Engine(prob, 3, lib=hip_lib)
    r = A.convert_scales(tab, sc.CM, ds[1:], T[1:], nH[1:])
    h = cols.height.copy()
    h[1:] = r.height
    A.set_columns(0, dataclasses.replace(cols, height=h))
    B.set_columns(0, cols)
    B.convert_scales(tab, 'column_mass', ds[1:], T[1:], nH[1:], col0=1, install=True, read_back=False)
    _equal(_one_fs(A), _one_fs(B))
    A.close(); B.close()


def test_install_keeps_populations_J_monitors_and_ng_state(hip_lib, falc):
    prob, block, _ = falc
    cols = _three(prob, block)
    ds, T, nH, ne = columns(sc.CM, 3)
    eng, twin = Engine(prob, 3, lib=hip_lib), Engine(prob, 3, lib=hip_lib)
    mon = []
    for e in (eng, twin):
        e.configure_ng(order=2)
        e.set_columns(0, cols)
        m = []
        for _ in range(3):
            m.append(e.formal_sol_gamma())
            m.append(e.stat_equil())
        mon.append(m)
    assert mon[0] == mon[1]
    state = lambda e: [e.get(w) for w in (_capi.LSX_N, _capi.LSX_J, _capi.LSX_DJ_COL, _capi.LSX_DPOPS_COL)]
    ng = lambda e: [getattr(e.ng_state(), k) for k in ('stored', 'applied', 'rejected', 'coef')]
    before, ng_before = state(eng), ng(eng)
    assert ng_before[0].max() > 0
    eng.convert_scales(sc.tables(), 'column_mass', ds, T, nH, install=True, read_back=False)
    for got in (state(eng), state(twin)):
        for x, y in zip(got, before):
            assert np.array_equal(x, y)
    for got in (ng(eng), ng(twin)):
        for x, y in zip(got, ng_before):
            assert np.array_equal(x, y)
    # the new heights are in: the next formal solution differs from the twin's
    assert eng.formal_sol_gamma() != twin.formal_sol_gamma()
    eng.close(); twin.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_change_nothing(hip_lib, falc):
    prob, block, _ = falc
    c = sc.Case('falc_cm')
    tab = sc.tables()
    eng, twin = Engine(prob, 2, lib=hip_lib), Engine(prob, 2, lib=hip_lib)

    def fails(code, *a, **k):
        with pytest.raises(_capi.LsxError) as e:
            eng.convert_scales(tab, *a, **k)
        assert e.value.code == code, e.value
        return str(e.value)
    EINVAL = _capi.LSX_EINVAL
    assert 'not set' in fails(EINVAL, sc.CM, c.ds, c.T, c.nH, install=True)                     # columns never set
    eng.set_columns(0, block)
    twin.set_columns(0, block); twin.set_columns(1, block)
    assert 'column 1' in fails(EINVAL, sc.CM, np.tile(c.ds, (2, 1)), np.tile(c.T, (2, 1)), np.tile(c.nH, (2, 1)), install=True)
    eng.set_columns(1, block)
    fails(EINVAL, sc.CM, c.ds, c.T, c.nH, col0=2, install=True)                                 # a bad column range
    fails(EINVAL, sc.CM, c.ds, c.T, c.nH, col0=-1, install=True)
    fails(EINVAL, sc.CM, np.tile(c.ds, (3, 1)), np.tile(c.T, (3, 1)), np.tile(c.nH, (3, 1)), install=True)
    fails(EINVAL, 7, c.ds, c.T, c.nH, install=True)                                             # a bad scale
    with pytest.raises(ValueError):
        eng.convert_scales(tab, 'mass', c.ds, c.T, c.nH)
    # non-monotonic scales
    h, tau = c.ref['height'][0], c.ref['tau_ref'][0]
    for scale, ds, ne in ((sc.CM, c.ds, None), (sc.TAU, tau, None), (sc.GEO, h, c.ne)):
        x = ds.copy()
        x[40] = x[39]
        assert 'depth_scale' in fails(EINVAL, scale, x, c.T, c.nH, ne, install=True)
        fails(EINVAL, scale, ds[::-1].copy(), c.T, c.nH, ne, install=True)
    T = c.T.copy()
    T[50] = 2400.0
    assert '2500' in fails(EINVAL, sc.CM, c.ds, T, c.nH, install=True)
    for bad in (np.nan, 0.0, -1.0, np.inf):
        fails(EINVAL, sc.CM, c.ds, np.where(np.arange(82) == 7, bad, c.T), c.nH, install=True)
        fails(EINVAL, sc.CM, c.ds, c.T, np.where(np.arange(82) == 7, bad, c.nH), install=True)
        fails(EINVAL, sc.GEO, h, c.T, c.nH, np.where(np.arange(82) == 7, bad, c.ne), install=True)
    # a cap that every point hits: LSX_ENOCONV names column and depth, nothing is installed
    with pytest.raises(_capi.LsxError) as e:
        eng.convert_scales(sc.tables().with_iter_cap(1), sc.CM, c.ds, c.T, c.nH, install=True)
    assert e.value.code == _capi.LSX_ENOCONV and 'column 0, depth 0' in str(e.value), e.value
    _equal(_one_fs(eng), _one_fs(twin))
    eng.close(); twin.close()


def test_one_depth_is_refused(hip_lib):
    """a depth scale needs two depths: no context of one depth exists (lsx_create), so neither the engine's entry nor the drop-in
    gets as far as a launch; the entry's own check of Nspace < 2 is covered on the host (tests/test_scales_host.py)"""
    c = sc.Case('s60_62_cm')
    a = StandIn(c)
    for k in ('depthScale', 'temperature', 'nHTot', 'ne'):
        setattr(a, k, getattr(a, k)[:1])
    with pytest.raises(_capi.LsxError) as e:
        lsa.convert_scales(a, sc.tables())
    assert e.value.code == _capi.LSX_EINVAL
    assert a.calls == ['nd', 'd'] and not hasattr(a, 'height')


def test_two_depths_make_a_context_but_no_formal_solution(hip_lib):
    eng = Engine(_carrier_problem(2), 1, lib=hip_lib)
    with pytest.raises(_capi.LsxError) as e:
        eng.formal_sol_gamma()
    assert e.value.code == _capi.LSX_EUNSUPPORTED
    eng.close()
