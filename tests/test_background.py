"""The background on the device (include/lsx_hip_background.h): lsx_hip_eos and lsx_hip_background against the UNMODIFIED
reference's numbers (tests/golden/background_eos.npz, and the bg_chi / bg_eta / bg_sca the committed FALC fixtures hold), inside
the bar of tests/background_cases.py; placement, chunking and the install path bit for bit; the errors; the drop-in Background.

Measured on MI355X (fraction of the bound, worst entry): see DESIGN.md 2, "how the background is pinned"."""
import numpy as np
import pytest

import background_cases as bc
from conftest import golden, relerr
from lightspinner_amd import Engine, _capi, fixtures, drivers
from lightspinner_amd.background import Background, _carrier_problem

pytestmark = pytest.mark.gpu


def carrier(hip_lib, Nspace):
    return Engine(_carrier_problem(Nspace), 1, lib=hip_lib)


@pytest.fixture(scope='module')
def falc():
    return fixtures.load_problem_npz(golden('falc_ca.npz'))


def perturbed(T, n, seed=5):
    """n columns: the given one and n - 1 with every temperature moved by up to 3 %"""
    rng = np.random.default_rng(seed)
    out = np.tile(T, (n, 1))
    out[1:] *= 1.0 + 0.03 * rng.uniform(-1, 1, (n - 1, T.shape[0]))
    return out


# ---- 1. the equation of state -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,shape', [('grid', (3, 22)), ('rf', (2, 82))])
def test_eos_against_the_reference(hip_lib, name, shape):
    d = bc.fixture()
    eng = carrier(hip_lib, shape[1])
    r = eng.eos(bc.tables(), d[name + '_temperature'].reshape(shape), d[name + '_nHTot'].reshape(shape))
    eng.close()
    assert np.array_equal(r.status, d[name + '_npepg'].reshape(shape))
    bc.inside(r.pgas, d[name + '_pgas'].reshape(shape), d[name + '_pgas_env'].reshape(shape), name + ' pgas')
    bc.inside(r.pe, d[name + '_pe'].reshape(shape), d[name + '_pe_env'].reshape(shape), name + ' pe')
    tr = lambda a: a.reshape(shape + (17,)).transpose(0, 2, 1)
    bc.inside(r.partials, tr(d[name + '_partials']), tr(d[name + '_partials_env']), name + ' partials')


# ---- 2. the background of one FALC column on the three grids, and the edges ---------------------------------------------------
@pytest.mark.parametrize('name', ['falc_ca.npz', 'falc_cah.npz', 'falc_all.npz'])
def test_background_of_falc(hip_lib, falc, name):
    g = np.load(golden(name))
    if name == 'falc_ca.npz':          # the context's own grid
        eng = Engine(falc[0], 1, lib=hip_lib)
        chi, eta, sca = eng.background(bc.tables(), g['temperature'], g['nHTot'], g['ne'])
    else:
        eng = carrier(hip_lib, 82)
        chi, eta, sca = eng.background(bc.tables(), g['temperature'], g['nHTot'], g['ne'], wavelength=g['wavelength'])
    eng.close()
    env = bc.falc_env_for(g['wavelength']) * np.abs(g['bg_chi'])
    bc.inside(chi[0], g['bg_chi'], env, name + ' chi')
    bc.inside(eta[0], g['bg_eta'], env * bc.planck(g['temperature'][None, :], g['wavelength'][:, None]), name + ' eta')
    ref_sca = g['bg_sca'] if g['bg_sca'].ndim == 1 else g['bg_sca'][0]
    assert np.all(np.abs(sca[0] - ref_sca) <= 4 * bc.U * np.abs(ref_sca))


def test_background_on_the_branch_grid_edges(hip_lib):
    d = bc.fixture()
    eng = carrier(hip_lib, 22)
    T, nH = d['grid_temperature'].reshape(3, 22), d['grid_nHTot'].reshape(3, 22)
    chi, eta, _ = eng.background(bc.tables(), T, nH, 1e-4 * nH, wavelength=d['grid_wavelength'])
    eng.close()
    nw = d['grid_wavelength'].shape[0]
    tr = lambda a: a.reshape(3, 22, nw).transpose(0, 2, 1)
    bc.inside(chi, tr(d['grid_chi']), tr(d['grid_chi_env']), 'grid chi (edges)')
    pl = bc.planck(T[:, None, :], d['grid_wavelength'][None, :, None])
    bc.inside(eta, tr(d['grid_chi']) * pl, tr(d['grid_chi_env']) * pl, 'grid eta (edges)')


# ---- 3. the 165 columns of the response function in one call ---------------------------------------------------------------
def test_response_function_columns_in_one_call(hip_lib):
    d = bc.fixture()
    g, rf = np.load(golden('falc_ca.npz')), np.load(golden('rf_ca_inputs.npz'))
    T = np.tile(g['temperature'], (165, 1))
    for k in range(82):
        T[1 + k, k] += 25.0
        T[83 + k, k] -= 25.0
    eng = carrier(hip_lib, 82)
    chi, eta, sca = eng.background(bc.tables(), T, np.tile(g['nHTot'], (165, 1)), np.tile(g['ne'], (165, 1)), wavelength=g['wavelength'])
    eng.close()
    env0 = bc.falc_env_for(g['wavelength']) * np.abs(g['bg_chi'])
    pl0 = bc.planck(g['temperature'][None, :], g['wavelength'][:, None])
    bc.inside(chi[0], g['bg_chi'], env0, 'base chi')
    bc.inside(eta[0], g['bg_eta'], env0 * pl0, 'base eta')
    mine_chi, mine_eta = np.zeros((164, 287)), np.zeros((164, 287))
    for c in range(164):
        k = c % 82
        others = np.arange(82) != k
        assert np.array_equal(chi[1 + c][:, others], chi[0][:, others]) and np.array_equal(eta[1 + c][:, others], eta[0][:, others])
        mine_chi[c], mine_eta[c] = chi[1 + c][:, k], eta[1 + c][:, k]
    ref_chi = np.array([rf['k%d%s_bg_chi' % (k, s)] for s in 'pm' for k in range(82)])
    ref_eta = np.array([rf['k%d%s_bg_eta' % (k, s)] for s in 'pm' for k in range(82)])
    env = bc.rel_env(d['rf_chi_env16']) * np.abs(ref_chi)
    bc.inside(mine_chi, ref_chi, env, 'rf chi')
    bc.inside(mine_eta, ref_eta, env * bc.planck(d['rf_temperature'][:, None], g['wavelength'][None, :]), 'rf eta')
    assert np.array_equal(sca, np.tile(sca[0], (165, 1)))


# ---- 4. placement and chunking, bit for bit ------------------------------------------------------------------------------------
def test_placement_and_wavelength_chunks_bit_for_bit(hip_lib):
    g = np.load(golden('falc_ca.npz'))
    w = g['wavelength']
    T = perturbed(g['temperature'], 7)
    T[3], T[6] = T[0], T[0]
    nH, ne = np.tile(g['nHTot'], (7, 1)), np.tile(g['ne'], (7, 1))
    eng = carrier(hip_lib, 82)
    tab = bc.tables()
    full = eng.background(tab, T, nH, ne, wavelength=w)
    alone = eng.background(tab, T[0], nH[0], ne[0], wavelength=w)
    for c in (0, 3, 6):
        for a, b in zip(full, alone):
            assert np.array_equal(a[c], b[0]), c
    part = eng.background(tab, T[2:5], nH[2:5], ne[2:5], wavelength=w)          # a column sub-range
    for a, b in zip(full, part):
        assert np.array_equal(a[2:5], b)
    for nla in (1, 63, 64, 65):
        chi, eta, _ = eng.background(tab, T[:2], nH[:2], ne[:2], wavelength=w[:nla])
        assert np.array_equal(chi, full[0][:2, :nla]) and np.array_equal(eta, full[1][:2, :nla]), nla
    eng.close()


def test_sixty_five_flattened_pairs(hip_lib):
    """5 columns x 13 depths: one (column, depth) pair more than a wave"""
    g = np.load(golden('falc_ca.npz'))
    idx = np.linspace(0, 81, 13).astype(int)
    T = perturbed(g['temperature'][idx], 5, seed=9)
    nH, ne = np.tile(g['nHTot'][idx], (5, 1)), np.tile(g['ne'][idx], (5, 1))
    w = g['wavelength'][::7]
    eng = carrier(hip_lib, 13)
    full = eng.background(bc.tables(), T, nH, ne, wavelength=w)
    e5 = eng.eos(bc.tables(), T, nH)
    for c in range(5):
        one = eng.background(bc.tables(), T[c], nH[c], ne[c], wavelength=w)
        e1 = eng.eos(bc.tables(), T[c], nH[c])
        for a, b in zip(full, one):
            assert np.array_equal(a[c], b[0]), c
        for key in ('pgas', 'pe', 'partials', 'status'):
            assert np.array_equal(getattr(e5, key)[c], getattr(e1, key)[0]), (c, key)
    eng.close()
    assert np.all(np.isfinite(full[0])) and np.all(full[0] > 0)


# ---- 5. install ----------------------------------------------------------------------------------------------------------------
def _three_columns(prob, block):
    from lightspinner_amd import ColumnBlock
    return ColumnBlock.concatenate([block, block, block]).validate(prob)


def _iterate(eng, n=3):
    mon = []
    for _ in range(n):
        mon.append(eng.formal_sol_gamma())
        mon.append(eng.stat_equil())
    return mon, [eng.get(w) for w in (_capi.LSX_I, _capi.LSX_J, _capi.LSX_GAMMA, _capi.LSX_N)]


def _same(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize('policy', ['ray-per-lane', 'ray-serial'])
def test_install_equals_set_columns_with_the_returned_arrays(hip_lib, falc, policy):
    import dataclasses
    prob, block, d = falc
    cols = _three_columns(prob, block)
    T = perturbed(d['temperature'], 3, seed=2)
    nH, ne = np.tile(d['nHTot'], (3, 1)), np.tile(d['ne'], (3, 1))
    A = Engine(prob, 3, lib=hip_lib, sweep_policy=policy)
    A.set_columns(0, cols)
    chi, eta, sca = A.background(bc.tables(), T, nH, ne, install=True)
    assert not np.array_equal(chi[0], chi[1])
    B = Engine(prob, 3, lib=hip_lib, sweep_policy=policy)
    B.set_columns(0, dataclasses.replace(cols, bg_chi=chi, bg_eta=eta, bg_sca=sca))
    assert A.sweep_policy() == B.sweep_policy() == policy
    _same(_iterate(A), _iterate(B))
    # an install later on leaves populations and J as they are; without read-back nothing comes back
    n0, J0 = A.get(_capi.LSX_N), A.get(_capi.LSX_J)
    assert A.background(bc.tables(), T[::-1].copy(), nH, ne, install=True, read_back=False) is None
    assert np.array_equal(A.get(_capi.LSX_N), n0) and np.array_equal(A.get(_capi.LSX_J), J0)
    A.close(); B.close()


def test_install_per_wavelength_scattering(hip_lib):
    import dataclasses
    import toy
    g = np.load(golden('falc_ca.npz'))
    prob, block = toy.toy_problem(sca_per_lambda=True, Nspace=37, ncol=3)
    nH = np.tile(np.geomspace(g['nHTot'].min(), g['nHTot'].max(), 37), (3, 1))
    ne = 1e-3 * nH
    A, B = Engine(prob, 3, lib=hip_lib), Engine(prob, 3, lib=hip_lib)
    A.set_columns(0, block)
    chi, eta, sca = A.background(bc.tables(), block.temperature, nH, ne, install=True)
    B.set_columns(0, dataclasses.replace(block, bg_chi=chi, bg_eta=eta, bg_sca=np.repeat(sca[:, None, :], prob.Nspect, axis=1).copy()))
    _same(_iterate(A), _iterate(B))
    A.close(); B.close()


def test_install_into_a_sub_range_leaves_the_other_columns_alone(hip_lib, falc):
    prob, block, d = falc
    cols = _three_columns(prob, block)
    T = perturbed(d['temperature'], 3, seed=2)
    C_, D_ = Engine(prob, 3, lib=hip_lib), Engine(prob, 3, lib=hip_lib)
    C_.set_columns(0, cols); D_.set_columns(0, cols)
    C_.background(bc.tables(), T[1:], np.tile(d['nHTot'], (2, 1)), np.tile(d['ne'], (2, 1)), col0=1, install=True, read_back=False)
    (_, rc), (_, rd) = _iterate(C_), _iterate(D_)
    for x, y in zip(rc, rd):
        assert np.array_equal(x[0], y[0])
    assert not np.array_equal(rc[1][2], rd[1][2])          # ... and the installed columns did change
    C_.close(); D_.close()


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------
def test_errors(hip_lib, falc):
    prob, block, d = falc
    T, nH, ne = d['temperature'], d['nHTot'], d['ne']
    eng, twin = Engine(prob, 2, lib=hip_lib), Engine(prob, 2, lib=hip_lib)
    tab = bc.tables()

    def einval(f, *a, **k):
        with pytest.raises(_capi.LsxError) as e:
            f(*a, **k)
        assert e.value.code == _capi.LSX_EINVAL, e.value
    for bad in (np.nan, np.inf, 0.0, -1.0):
        for which in range(3):
            arrs = [T.copy(), nH.copy(), ne.copy()]
            arrs[which][17] = bad
            einval(eng.background, tab, *arrs)
        einval(eng.eos, tab, np.where(np.arange(82) == 3, bad, T), nH)
    fx = bc.fixture()
    mk = lambda **kw: bc.EosTables(**{**dict(tpf=fx['tpf'], pf=fx['pf'], eion=fx['eion'], nstage=fx['nstage'], abund=fx['abund'],
                                             amass=fx['amass'], weight_per_H=float(fx['weight_per_H'])), **kw})
    einval(eng.eos, mk(nstage=fx['nstage'][:27], pf=fx['pf'][:27], eion=fx['eion'][:27]), T, nH)          # nelem < 28
    tpf = fx['tpf'].copy(); tpf[5] = tpf[4]
    einval(eng.eos, mk(tpf=tpf), T, nH)
    for e, v in ((3, 0), (3, 7), (1, 2), (19, 1), (0, 1)):          # outside 1..6; He, Ca, H with fewer stages than are read
        ns = fx['nstage'].copy(); ns[e] = v
        einval(eng.eos, mk(nstage=ns), T, nH)
    einval(eng.background, tab, T, nH, ne, wavelength=[500.0, 400.0])
    einval(eng.background, tab, T, nH, ne, wavelength=[-1.0, 400.0])
    einval(eng.background, tab, T, nH, ne, wavelength=[500.0], install=True)
    einval(eng.background, tab, T, nH, ne, install=True)                       # columns never set
    eng.set_columns(0, block); eng.set_columns(1, block)
    twin.set_columns(0, block); twin.set_columns(1, block)
    einval(eng.background, tab, T, nH, ne, col0=2, install=True)               # a bad column range
    einval(eng.background, tab, np.tile(T, (3, 1)), np.tile(nH, (3, 1)), np.tile(ne, (3, 1)), install=True)
    # a cap that every point hits: LSX_ENOCONV names column and depth, nothing is installed
    with pytest.raises(_capi.LsxError) as e:
        eng.background(bc.tables(iter_cap=2), perturbed(T, 2), np.tile(nH, (2, 1)), np.tile(ne, (2, 1)), install=True)
    assert e.value.code == _capi.LSX_ENOCONV and 'column 0, depth 0' in str(e.value), e.value
    with pytest.raises(_capi.LsxError) as e:
        eng.eos(bc.tables(iter_cap=2), T, nH)
    assert e.value.code == _capi.LSX_ENOCONV and np.all(e.value.result.status < 0)
    _same(_iterate(eng), _iterate(twin))
    eng.close(); twin.close()


# ---- 7. the drop-in Background ---------------------------------------------------------------------------------------------------
def test_background_object_drives_the_context(hip_lib):
    from helpers import build_fakes
    from lightspinner_amd.rh_method import Context
    d = dict(np.load(golden('falc_ca.npz')))
    prob, _, _ = fixtures.load_problem_npz(d)
    atmos, spect, eq, _ = build_fakes(d)
    bg = Background(atmos, spect, bc.tables())
    assert bg.chi.shape == bg.eta.shape == bg.sca.shape == (prob.Nspect, prob.Nspace)
    ctx = Context(atmos, spect, eq, bg, lib=hip_lib)
    h = drivers.iterate_mali(ctx)
    assert h.converged and h.n_iter == 46
    n = np.concatenate([a.n for a in ctx.activeAtoms])
    assert relerr(n, fixtures.pops_from_raw(d, 'conv', prob)) < 1e-6
    assert relerr(ctx.J, d['conv_J']) < 1e-6 and relerr(ctx.I, d['conv_I']) < 1e-6
    ctx.close()
