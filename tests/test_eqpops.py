"""LTE populations of any atoms on the device (include/lsx_hip_eqpops.h): lsx_hip_eq_pops against the committed fixtures of the
unmodified reference and against the CPU build of the same header, inside the set-up chain's bar (tests/eqpops_cases.py); thread
counts around the wave and the block size with placement bit for bit; nTotal left out; and, for an atom that is active in a
context, the bits lsx_set_atmosphere(lte_pops=1) leaves in LSX_NSTAR, with the context untouched.

Thread counts: one thread per (column, depth), 128 per block.  A context has at least two depths, so ncol x Nspace = 1 cannot be
formed; 2 stands in for it (2-depth carrier), 64 = 32 x 2, 3 and 63 on the 3-depth carrier, 65 = 5 x 13, 257 on a 257-depth one,
and 164 / 574 = 2 / 7 x 82."""
import numpy as np
import pytest

import eqpops_cases as ec
from conftest import golden
from setup_cases import Ledger
from lightspinner_amd import ColumnBlock, Engine, _capi, atomdata, fixtures
from lightspinner_amd.background import _carrier_problem

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in ec.all_cases()}


@pytest.fixture(scope='module')
def carriers(hip_lib):
    made = {}

    def get(Nspace):
        if Nspace not in made:
            made[Nspace] = Engine(_carrier_problem(Nspace), 1, lib=hip_lib)
        return made[Nspace]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope='module')
def host():
    return ec.HostLib()


def device(eng, case, **kw):
    return eng.eq_pops(case.atoms, case.ab, case.T, case.ne, case.nH, **kw)


# ---- 1. against the fixtures and the host build ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_against_the_fixtures_and_the_host_build(carriers, host, name):
    c = CASES[name]
    r = device(carriers(82), c)
    led = Ledger('HIP ' + name)
    ec.check_case(led, c, r)
    h = host.of_case(c)
    for a, atom in enumerate(c.atoms):
        ec.check(led, 'vs host', r.nStar[a], h.nStar[a], atom, c.T, factor=2.0)
        print('%s %s: %s the host build' % (name, atom.name, 'bit-equal to' if np.array_equal(r.nStar[a], h.nStar[a]) else 'not bit-equal to'))
    assert np.array_equal(r.nTotal, h.nTotal)
    led.report()


def test_hydrogen_alone_on_falc(carriers):
    c = CASES['falc_atm0']
    r = carriers(82).eq_pops(c.atoms[:1], c.ab[:1], c.T[0], c.ne[0], c.nH[0])
    assert r.nStar[0].shape == (1, 6, 82) and r.nTotal.shape == (1, 1, 82)
    led = Ledger('HIP hydrogen')
    ec.check(led, 'nStar', r.nStar[0], c.ref[0], c.atoms[0], c.T)
    ec.check(led, 'hGround', r.nStar[0][:, :1], c.hGround[:, None], c.atoms[0], c.T, rows=slice(0, 1))
    assert np.array_equal(r.nStar[0], device(carriers(82), c).nStar[0])          # alone = beside calcium
    led.report()


def test_made_up_atoms(carriers, host):
    toys = ec.toy_atoms()
    T, ne, nH = ec.toy_atmosphere()
    names = list(toys)
    atoms, ab = [toys[n][0] for n in names], [toys[n][1] for n in names]
    r = carriers(13).eq_pops(atoms, ab, T, ne, nH)
    rc, h = host.eq_pops(atoms, ab, T, ne, nH)
    assert rc == 0
    led = Ledger('HIP toys')
    for a, n in enumerate(names):
        ec.check(led, n, r.nStar[a], np.moveaxis(ec.lte_numpy(atoms[a], T, ne, ab[a] * nH), 0, 1), atoms[a], T)
        ec.check(led, n + ' vs host', r.nStar[a], h.nStar[a], atoms[a], T, factor=2.0)
    assert np.array_equal(r.nStar[names.index('one')][:, 0], nH)
    assert np.all(r.nStar[names.index('absent')] == 0.0)
    assert np.array_equal(r.nTotal, h.nTotal)
    led.report()


# ---- 2. thread counts and placement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Ns,ncol', [(2, 1), (3, 1), (3, 21), (2, 32), (13, 5), (257, 1), (82, 2), (82, 7)])
def test_thread_counts_and_placement(carriers, Ns, ncol):
    s = ec._npz('setup_atoms.npz')
    atoms, ab = ec.fixture_atoms(s)
    rng = np.random.default_rng(Ns * 1000 + ncol)
    nrow = max(7, ncol)
    pick = lambda a: np.resize(a, nrow * Ns).reshape(nrow, Ns) * rng.uniform(0.9, 1.1, (nrow, Ns))
    T, ne, nH = pick(s['edge_temperature'][20:60]), pick(s['edge_ne'][20:60]), pick(s['edge_nHTot'][20:60])
    eng = carriers(Ns)
    r = eng.eq_pops(atoms, ab, T[:ncol], ne[:ncol], nH[:ncol])
    assert np.all(np.isfinite(r.nStar_flat)) and r.nStar_flat.shape == (ncol, 53, Ns)
    led = Ledger('HIP %d threads' % (Ns * ncol))
    for a, atom in enumerate(atoms):
        ec.check(led, 'nStar', r.nStar[a], np.moveaxis(ec.lte_numpy(atom, T[:ncol], ne[:ncol], ab[a] * nH[:ncol]), 0, 1), atom, T[:ncol])
    # the last column alone, and as column 0, 3 and 6 of seven
    c = ncol - 1
    alone = eng.eq_pops(atoms, ab, T[c], ne[c], nH[c])
    assert np.array_equal(alone.nStar_flat[0], r.nStar_flat[c]) and np.array_equal(alone.nTotal[0], r.nTotal[c])
    order = [c, 1, 2, c, 4, 5, c]
    seven = eng.eq_pops(atoms, ab, T[order], ne[order], nH[order])
    for q in (0, 3, 6):
        assert np.array_equal(seven.nStar_flat[q], alone.nStar_flat[0]) and np.array_equal(seven.nTotal[q], alone.nTotal[0]), q
    # nTotal left out
    bare = eng.eq_pops(atoms, ab, T[:ncol], ne[:ncol], nH[:ncol], want_nTotal=False)
    assert bare.nTotal is None and np.array_equal(bare.nStar_flat, r.nStar_flat)
    led.report()


# ---- 3. an atom that is active in a context ------------------------------------------------------------------------------------------
def test_active_atom_gets_the_bits_of_set_atmosphere_and_the_context_is_untouched(hip_lib):
    d = ec._npz('setup_falc.npz')
    prob, block, raw = fixtures.load_problem_npz(golden('falc_ca.npz'))
    atoms, ab = ec.fixture_atoms(d)
    data = atomdata.from_fixture(d, atoms=[1])
    c = CASES['rf_164']                                   # two perturbed atmospheres
    e = Engine(prob, 2, lib=hip_lib)
    e.set_columns(0, ColumnBlock.concatenate([block, block]))
    e.set_atomic_data(data)
    two = lambda a: np.stack([a, a])
    e.set_atmosphere(0, c.T, c.ne, two(raw['vturb']), c.hGround, (ab[1] * c.nH)[:, None], lte_pops=True)
    for _ in range(4):
        e.formal_sol_gamma()
    e.stat_equil()
    before = {w: e.get(w) for w in (_capi.LSX_I, _capi.LSX_J, _capi.LSX_N, _capi.LSX_NSTAR, _capi.LSX_GAMMA)}
    r = e.eq_pops(atoms, ab, c.T, c.ne, c.nH)
    assert np.array_equal(r.nStar[1], before[_capi.LSX_NSTAR])
    alone = e.eq_pops(atoms[1:], ab[1:], c.T, c.ne, c.nH)
    assert np.array_equal(alone.nStar[0], before[_capi.LSX_NSTAR]) and np.array_equal(alone.nTotal[:, 0], ab[1] * c.nH)
    for w, v in before.items():
        assert np.array_equal(e.get(w), v), w
    dJ = e.formal_sol_gamma()
    # the same call sequence without eq_pops in between
    e2 = Engine(prob, 2, lib=hip_lib)
    e2.set_columns(0, ColumnBlock.concatenate([block, block]))
    e2.set_atomic_data(data)
    e2.set_atmosphere(0, c.T, c.ne, two(raw['vturb']), c.hGround, (ab[1] * c.nH)[:, None], lte_pops=True)
    for _ in range(4):
        e2.formal_sol_gamma()
    e2.stat_equil()
    assert e2.formal_sol_gamma() == dJ
    for w in (_capi.LSX_I, _capi.LSX_J, _capi.LSX_N):
        assert np.array_equal(e.get(w), e2.get(w)), w
    e.close()
    e2.close()


def test_errors_reach_python(carriers):
    c = CASES['falc_atm0']
    T = c.T.copy()
    T[0, 7] = -1.0
    with pytest.raises(_capi.LsxError, match='lsx_hip_eq_pops.*depth 7'):
        carriers(82).eq_pops(c.atoms, c.ab, T, c.ne, c.nH)
    with pytest.raises(ValueError):
        carriers(82).eq_pops(c.atoms, c.ab[:1], c.T, c.ne, c.nH)
    with pytest.raises(ValueError):
        carriers(82).eq_pops(c.atoms, c.ab, c.T, c.ne[:, :40], c.nH)


# ---- the drop-in table ------------------------------------------------------------------------------------------------------------------
def test_drop_in_table_drives_a_context(hip_lib):
    """eqpops.compute_eq_pops on Lightspinner-shaped models: what rh_method.Context reads of the table (eqPops['H'].n[0], the active
    atom's nStar / nTotal / pops) is there, and the FALC CaII run on it converges as the reference's does"""
    from helpers import build_fakes, _Element, _Level
    from lightspinner_amd import drivers
    from lightspinner_amd.eqpops import compute_eq_pops
    from lightspinner_amd.rh_method import Context
    d, s = dict(np.load(golden('falc_ca.npz'))), ec._npz('setup_falc.npz')
    atmos, spect, _, bg = build_fakes(d)
    atmos.dimensioned = True
    names = [str(x) for x in s['atom_names']]
    table = {n: _Element(s['m%d_weight' % m], s['m%d_abundance' % m]) for m, n in enumerate(names)}

    class Model:
        def __init__(self, m):
            self.name, self.atomicTable = names[m], table
            self.levels = [_Level(*q) for q in zip(s['m%d_lev_E_SI' % m], s['m%d_lev_g' % m], s['m%d_lev_stage' % m])]
    eq = compute_eq_pops([Model(1), Model(0)], atmos)                 # any order in: atomic-weight order out
    assert [a.name for a in eq] == ['H', 'CA'] and len(eq) == 2 and 'Ca' in eq and 'ca' in eq and 'Fe' not in eq
    assert atmos.nondim_calls == 1 and eq.atomicTable is table
    c = CASES['falc_atm0']
    led = Ledger('drop-in')
    ec.check(led, 'H', eq['H'].nStar[None], c.ref[0], c.atoms[0], c.T)
    ec.check(led, 'Ca', eq['Ca'].nStar[None], c.ref[1], c.atoms[1], c.T)
    assert np.array_equal(eq['CA'].nTotal, d['a0_nTotal']) and eq['CA'].pops is None and eq['H'].n is eq['H'].nStar
    ctx = Context(atmos, spect, eq, bg)
    h = drivers.iterate_mali(ctx)
    assert h.n_iter == int(d['n_iter']) == 46
    assert ctx.activeAtoms[0].n is eq['Ca'].pops and eq['Ca'].n is eq['Ca'].pops
    from conftest import relerr
    assert relerr(eq['Ca'].pops, d['conv_n_a0']) < 1e-6 and relerr(ctx.I, d['conv_I']) < 1e-6
    ctx.close()
    led.report()
