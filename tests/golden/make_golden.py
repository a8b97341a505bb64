#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ by importing the UNMODIFIED
reference from /root/reference (build container only; the reference never
travels to the GPU box -- only the numeric .npz files written here do).

The reference imports numba / astropy / specutils at module top; none is
installed in this image, so harness-side stand-ins from tests/golden/_refstubs
are put on sys.path (numba.njit == identity, i.e. the reference's pure-Python
semantics).  One numpy-2 compatibility patch is applied at run time, nothing
under /root/reference is touched:
  * atomic_model.avoid_recursion_eq     returns False for shape-mismatched
    arrays (numpy<1.25 semantics; only used for list membership in setup).
(np.bool, used at rh_method.py:124, exists again in numpy 2.x.)

Usage:  python tests/golden/make_golden.py [units] [falc_ca] [falc_cah] [falc_ca_vlos] [falc_c] [falc_fe] [falc_mg] [falc_all] [rf] [rf_inputs] [rf_outputs] [setup] [live_ref] [setup_atoms] [all]
        python tests/golden/make_topology_golden.py [toy] [rs] [inst] [shallow] [bare] [dead] [all]      (topologies_*.npz: the made-up topologies)
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('LIGHTSPINNER_REF', '/root/reference')
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, '_refstubs'))
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

import atomic_model  # noqa: E402

_orig_eq = atomic_model.avoid_recursion_eq


def _compat_eq(a, b):
    if isinstance(a, np.ndarray):
        if not isinstance(b, np.ndarray) or a.shape != b.shape:
            return False
    return _orig_eq(a, b)


atomic_model.avoid_recursion_eq = _compat_eq

import formal_solver  # noqa: E402
from fal import Falc82  # noqa: E402
from rh_atoms import CaII_atom, H_6_atom, C_atom, Fe_simple_atom, MgII_atom  # noqa: E402
from atomic_set import RadiativeSet  # noqa: E402
from rh_method import Context  # noqa: E402
from background import Background  # noqa: E402
from atomic_model import AtomicLine  # noqa: E402


# ----------------------------------------------------------------------------
def build_ctx(active, vlos=None, temp_pert=None, start_pops=None, nrays=5, models=None):
    """Reproduces the setup of test.py:8-18 / response_fn.py:23-37.  models: the RadiativeSet's atomic models (default: test.py's
    CaII + H); hydrogen must be among them (its ground-level populations enter the van der Waals damping, rh_method.py:223)."""
    ac = Falc82()
    ac.quadrature(nrays)
    if temp_pert is not None:
        k, dT = temp_pert
        ac.temperature[k] += dT  # Quantity in K; same as response_fn.py:26
    if vlos is not None:
        ac.vlos[:] = vlos  # m/s (constructor already converted to SI)
    atmos = ac.convert_scales()
    aSet = RadiativeSet(models if models is not None else [CaII_atom(), H_6_atom()])
    aSet.set_active(*active)
    spect = aSet.compute_wavelength_grid()
    eqPops = aSet.compute_eq_pops(atmos)
    if start_pops is not None:
        for name, p in start_pops.items():
            eqPops[name].pops = np.copy(p)
    background = Background(atmos, spect)
    ctx = Context(atmos, spect, eqPops, background)
    return ctx


def dump_inputs(ctx, full_phi=False, phi_sample_only=False):
    """Flat dict of the post-setup hot-path inputs."""
    atmos, spect, bg = ctx.atmos, ctx.spect, ctx.background
    d = {}
    d['wavelength'] = np.array(spect.wavelength)
    for k in ('muz', 'wmu', 'height', 'temperature', 'ne', 'vlos', 'vturb', 'nHTot'):
        d[k] = np.array(getattr(atmos, k), dtype=np.float64)
    d['bg_chi'] = np.array(bg.chi)
    d['bg_eta'] = np.array(bg.eta)
    sca = np.array(bg.sca)
    if np.all(sca == sca[0:1]):
        d['bg_sca'] = sca[0].copy()
    else:
        d['bg_sca'] = sca
    d['hGround'] = np.array(ctx.eqPops['H'].n[0])
    names = []
    t_atom, t_isline, t_i, t_j, t_nblue, t_nl = [], [], [], [], [], []
    t_A, t_Bji, t_Bij, t_l0 = [], [], [], []
    t_active = []
    kr = 0
    for a, atom in enumerate(ctx.activeAtoms):
        # compute_collisions is re-run at the top of every FS call; C is a pure
        # function of the atmosphere (rh_method.py:474-487), capture it here.
        atom.compute_collisions()
        names.append(atom.atomicModel.name)
        d['a%d_nStar' % a] = np.array(atom.nStar)
        d['a%d_nTotal' % a] = np.array(atom.nTotal)
        d['a%d_n0' % a] = np.array(atom.n)
        d['a%d_C' % a] = np.array(atom.C)
        d['a%d_vBroad' % a] = np.array(atom.vBroad)
        d['a%d_weight' % a] = np.float64(atom.atomicTable[atom.atomicModel.name].weight)
        for t in atom.trans:
            t_atom.append(a)
            t_isline.append(1 if t.isLine else 0)
            t_i.append(t.i)
            t_j.append(t.j)
            t_nblue.append(int(t.Nblue))
            t_nl.append(t.wavelength.shape[0])
            t_active.append(np.array(t.active, dtype=np.bool_))
            d['t%d_wavelength' % kr] = np.array(t.wavelength)
            if t.isLine:
                t_A.append(t.Aji); t_Bji.append(t.Bji); t_Bij.append(t.Bij); t_l0.append(t.lambda0)
                d['t%d_wphi' % kr] = np.array(t.wphi)
                aDamp, _ = t.transModel.damping(atmos, atom.vBroad, atom.hPops.n[0])
                d['t%d_aDamp' % kr] = np.array(aDamp)
                phi = np.array(t.phi)
                same = np.all(phi == phi[:, :1, :1, :])
                if phi_sample_only:
                    d['t%d_phi_sample' % kr] = phi[::7, :, :, ::9].copy()
                elif same and not full_phi:
                    d['t%d_phi' % kr] = phi[:, 0, 0, :].copy()
                else:
                    d['t%d_phi' % kr] = phi
            else:
                t_A.append(0.0); t_Bji.append(0.0); t_Bij.append(0.0); t_l0.append(0.0)
                d['t%d_alpha' % kr] = np.array(t.alpha)
            kr += 1
    d['atom_names'] = np.array(names)
    d['t_atom'] = np.array(t_atom, dtype=np.int32)
    d['t_isline'] = np.array(t_isline, dtype=np.int32)
    d['t_i'] = np.array(t_i, dtype=np.int32)
    d['t_j'] = np.array(t_j, dtype=np.int32)
    d['t_Nblue'] = np.array(t_nblue, dtype=np.int32)
    d['t_Nlambda'] = np.array(t_nl, dtype=np.int32)
    d['t_Aji'] = np.array(t_A); d['t_Bji'] = np.array(t_Bji)
    d['t_Bij'] = np.array(t_Bij); d['t_lambda0'] = np.array(t_l0)
    d['t_active'] = np.array(t_active)
    return d


def snap_fs(ctx, d, tag, dJ, with_rates=False):
    d['%s_J' % tag] = ctx.J.copy()
    d['%s_I' % tag] = ctx.I.copy()
    d['%s_dJ' % tag] = np.float64(dJ)
    for a, atom in enumerate(ctx.activeAtoms):
        d['%s_Gamma_a%d' % (tag, a)] = atom.Gamma.copy()
    if with_rates:
        kr = 0
        for atom in ctx.activeAtoms:
            for t in atom.trans:
                d['%s_Rij_t%d' % (tag, kr)] = t.Rij.copy()
                d['%s_Rji_t%d' % (tag, kr)] = t.Rji.copy()
                kr += 1


def snap_se(ctx, d, tag, dPops):
    d['%s_dPops' % tag] = np.float64(dPops)
    for a, atom in enumerate(ctx.activeAtoms):
        d['%s_n_a%d' % (tag, a)] = atom.n.copy()


def run_mali(ctx, d, snap_iters=(1, 2, 3, 4, 5), max_iter=500, stop_after=None, log=None):
    """The driver loop of test.py:20-29 with snapshots."""
    dJ, dPops, i = 1.0, 1.0, 0
    traj_dJ, traj_dP = [], []
    t0 = time.time()
    while dJ > 2e-3 or dPops > 1e-3:
        i += 1
        dJ = ctx.formal_sol_gamma_matrices()
        if i in snap_iters:
            snap_fs(ctx, d, 'fs%d' % i, dJ, with_rates=(i <= 2))
        if i > 3:
            dPops = ctx.stat_equil()
            if i in snap_iters:
                snap_se(ctx, d, 'se%d' % i, dPops)
        traj_dJ.append(dJ)
        traj_dP.append(dPops if i > 3 else np.nan)
        if log:
            print('%s it %03d dJ %.6e dPops %.6e  (%.1fs)' % (log, i, dJ, dPops, time.time() - t0), flush=True)
        if stop_after is not None and i >= stop_after:
            break
        if i >= max_iter:
            break
    d['traj_dJ'] = np.array(traj_dJ)
    d['traj_dPops'] = np.array(traj_dP)
    d['n_iter'] = np.int32(i)
    return i


def save(name, d):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **d)
    print('wrote %s (%.1f kB)' % (path, os.path.getsize(path) / 1e3), flush=True)


# ----------------------------------------------------------------------------
def gen_units():
    """w2 / piecewise_1d_impl / piecewise_linear_1d / planck unit vectors."""
    from utils import planck
    d = {}
    dt = np.concatenate([np.logspace(-12, 9, 400),
                         [5e-4, np.nextafter(5e-4, 0), np.nextafter(5e-4, 1),
                          50.0, np.nextafter(50.0, 0), np.nextafter(50.0, 100.0), 0.0]])
    d['w2_dtau'] = dt
    d['w2_out'] = np.array([formal_solver.w2(x) for x in dt])
    rng = np.random.default_rng(20260101)
    cases = []
    for c, N in enumerate([3, 4, 5, 17, 82, 82, 82, 83, 200, 41]):
        z = np.sort(rng.uniform(-1e5, 2e6, N))[::-1].copy()
        logchi = np.cumsum(rng.normal(0.15, 0.3, N)) + rng.uniform(-16, -9)
        chi = np.exp(logchi)
        if c == 5:
            chi *= 1e6  # mostly saturated branch
        if c == 6:
            chi *= 1e-6  # mostly Taylor branch
        S = np.exp(rng.normal(-20, 1.0, N)) * np.linspace(0.1, 3.0, N)
        mu = float(rng.uniform(0.04, 1.0))
        for toFrom in (False, True):
            Istart = float(rng.uniform(0, 1e-8)) if toFrom else 0.0
            I, Psi = formal_solver.piecewise_1d_impl(mu, toFrom, Istart, z, chi, S)
            tag = 'pw%d_%d' % (c, int(toFrom))
            d[tag + '_z'] = z; d[tag + '_chi'] = chi; d[tag + '_S'] = S
            d[tag + '_mu'] = np.float64(mu); d[tag + '_Istart'] = np.float64(Istart)
            d[tag + '_I'] = I; d[tag + '_Psi'] = Psi
        cases.append(N)
    d['pw_N'] = np.array(cases, dtype=np.int32)

    # piecewise_linear_1d with boundary conditions on a duck-typed atmosphere
    class A:
        pass
    at = A()
    at.Nspace = 82
    at.muz = np.array([0.2, 0.9])
    at.height = np.sort(rng.uniform(-1e5, 2e6, 82))[::-1].copy()
    at.temperature = np.linspace(4000.0, 9500.0, 82)
    chi = np.exp(np.cumsum(rng.normal(0.2, 0.3, 82)) - 14)
    S = np.exp(rng.normal(-19, 0.5, 82))
    d['pl_height'] = at.height; d['pl_temperature'] = at.temperature; d['pl_muz'] = at.muz
    d['pl_chi'] = chi; d['pl_S'] = S
    wavs = np.array([30.0, 393.4, 854.2, 2000.0])
    d['pl_wav'] = wavs
    for wi, wav in enumerate(wavs):
        for mu in range(2):
            for toFrom in (False, True):
                r = formal_solver.piecewise_linear_1d(at, mu, toFrom, wav, chi, S)
                d['pl_I_%d_%d_%d' % (wi, mu, int(toFrom))] = r.I
                d['pl_Psi_%d_%d_%d' % (wi, mu, int(toFrom))] = r.PsiStar
    T = np.array([3000.0, 4500.0, 6000.0, 9000.0, 1e5])
    d['planck_T'] = T
    d['planck_wav'] = wavs
    d['planck_B'] = np.array([planck(T, w) for w in wavs])
    save('units.npz', d)


def gen_falc_ca():
    ctx = build_ctx(['Ca'])
    d = dump_inputs(ctx)
    n = run_mali(ctx, d, log='falc_ca')
    snap_fs(ctx, d, 'conv', d['traj_dJ'][-1])
    snap_se(ctx, d, 'conv', d['traj_dPops'][-1])
    print('falc_ca converged in', n)
    save('falc_ca.npz', d)
    return ctx


def gen_falc_cah(stop_after=8):
    ctx = build_ctx(['Ca', 'H'])
    d = dump_inputs(ctx)
    run_mali(ctx, d, snap_iters=(1, 2, 4, 5), stop_after=stop_after, log='falc_cah')
    snap_fs(ctx, d, 'last', d['traj_dJ'][-1])
    snap_se(ctx, d, 'last', d['traj_dPops'][-1])
    # keep the fixture small: drop the bulky intermediate J snapshots except fs1/fs2/last
    for k in list(d.keys()):
        if k in ('fs4_J', 'fs5_J'):
            del d[k]
    save('falc_cah.npz', d)


def gen_falc_ca_vlos():
    """Non-zero line-of-sight velocity: phi is genuinely 4-D (rh_method.py:229-240).
    Only the ingredients of phi (aDamp, vBroad, vlos) plus a strided sample of the
    reference's phi are stored; tests rebuild phi with the same scipy wofz."""
    k = np.arange(82)
    vlos = 4.0e3 * np.sin(2 * np.pi * k / 41.0) * np.exp(-((k - 35.0) / 25.0) ** 2) + 1.5e3
    ctx = build_ctx(['Ca'], vlos=vlos)
    d = dump_inputs(ctx, phi_sample_only=True)
    run_mali(ctx, d, snap_iters=(1, 2, 4, 5), stop_after=6, log='falc_ca_vlos')
    snap_fs(ctx, d, 'last', d['traj_dJ'][-1])
    snap_se(ctx, d, 'last', d['traj_dPops'][-1])
    # the unperturbed-layout quantities identical to falc_ca are kept (file is self-contained)
    save('falc_ca_vlos.npz', d)


def gen_falc_multilevel(which):
    """FALC with one of the reference's larger model atoms active (rh_atoms.py:194 C_atom: 15 levels, 16 lines, 14 bound-free
    continua onto C II; :355 Fe_simple_atom: 15 levels, 15 lines, 14 continua; :50 MgII_atom: 11 levels, 15 lines, 10 continua):
    up to 14 transitions overlap at a wavelength, every continuum shares its atom with the lines it overlaps
    (rh_method.py:606-627, 654-681: the atom.eta / atom.chi / atom.U cross terms between lines and continua of one atom).
    Inputs + J, I, Gamma, dJ after formal solutions 1-4 and n, dPops after the first statistical equilibrium."""
    ctor, name = {'c': (C_atom, 'C'), 'fe': (Fe_simple_atom, 'Fe'), 'mg': (MgII_atom, 'MG')}[which]
    ctx = build_ctx([name], models=[H_6_atom(), ctor()])
    d = dump_inputs(ctx)
    run_mali(ctx, d, snap_iters=(1, 2, 3, 4), stop_after=4, log='falc_' + which)
    for k in ('fs2_J', 'fs3_J'):          # keep the file small: J after calls 1 and 4 (fs1_J is the J-dagger of call 2, and so on)
        del d[k]
    for k in list(d.keys()):              # the rates' snapshots pin I at every depth: keep them for call 1 only
        if k.startswith('fs2_R'):
            del d[k]
    save('falc_%s.npz' % which, d)


def gen_falc_all():
    """FALC with ALL FIVE of the reference's model atoms in the set and active at once (rh_atoms.py:4 H_6, :50 MgII, :152 CaII,
    :194 C, :355 Fe_simple): 53 levels, 109 transitions, up to 44 bound-free continua of five atoms overlap at a wavelength, five Gamma matrices and five
    statistical equilibria per iteration (rh_method.py:586-590 the loop over the active atoms at a wavelength, :710 over the atoms
    of a statistical equilibrium).  Inputs + I, Gamma, dJ after formal solutions 1 and 4, J after 4, n and dPops after the first
    statistical equilibrium."""
    ctx = build_ctx(['H', 'Ca', 'MG', 'C', 'Fe'], models=[H_6_atom(), CaII_atom(), MgII_atom(), C_atom(), Fe_simple_atom()])
    d = dump_inputs(ctx)
    run_mali(ctx, d, snap_iters=(1, 4), stop_after=4, log='falc_all')
    del d['fs1_J']
    for k in list(d.keys()):
        if k.startswith('fs1_R'):
            del d[k]
    save('falc_all.npz', d)


def gen_rf(ks=(20, 48, 70)):
    """response_fn.py:23-67 for a handful of depth indices: delta-encoded inputs
    (only the depth-k entries differ) + converged emergent I."""
    base = build_ctx(['Ca'])
    dbase = dump_inputs(base)
    tmp = {}
    run_mali(base, tmp, snap_iters=(), log='rf_base')
    out = {'ks': np.array(ks, dtype=np.int32), 'tempPert': np.float64(50.0)}
    out['base_I'] = base.I.copy()
    out['base_n'] = base.activeAtoms[0].n.copy()
    out['base_niter'] = tmp['n_iter']
    startPops = {'Ca': base.eqPops['Ca'].n}
    for k in ks:
        for sgn, tag in ((+1, 'p'), (-1, 'm')):
            ctx = build_ctx(['Ca'], temp_pert=(k, sgn * 25.0), start_pops=startPops)
            dp = dump_inputs(ctx)
            # delta encode: store every array that differs from base, verifying where it differs
            for key, v in dp.items():
                b = dbase[key]
                if v.dtype.kind in 'US' or v.dtype.kind in 'ib':
                    assert np.array_equal(v, b), key
                    continue
                if key.endswith('_n0'):
                    continue  # warm start = base_n
                if np.array_equal(v, b):
                    continue
                diff = (v != b)
                where_k = np.zeros_like(diff)
                where_k[..., k] = True
                if key == 'height':
                    # uniform shift only: |dz| must be bitwise identical
                    assert np.array_equal(np.diff(v), np.diff(b)), 'height diff changed'
                    continue
                assert not np.any(diff & ~where_k), 'non-local change in %s' % key
                out['k%d%s_%s' % (k, tag, key)] = v[..., k].copy()
            t2 = {}
            n = run_mali(ctx, t2, snap_iters=(), log='rf_k%d%s' % (k, tag))
            out['k%d%s_I' % (k, tag)] = ctx.I.copy()
            out['k%d%s_n' % (k, tag)] = ctx.activeAtoms[0].n.copy()
            out['k%d%s_niter' % (k, tag)] = np.int32(n)
            out['k%d%s_traj_dJ' % (k, tag)] = t2['traj_dJ']
            out['k%d%s_traj_dPops' % (k, tag)] = t2['traj_dPops']
    save('rf_ca.npz', out)


def gen_rf_inputs(out_name='rf_ca_inputs.npz'):
    """response_fn.py:23-57, the INPUTS of all 2 x Nspace perturbed runs (T[k] +- 25 K), delta-encoded against the
    unperturbed column like gen_rf (only depth-k entries differ).  No converged reference outputs: running the
    reference's 164 MALI loops is hours of pure Python; parity of the response function is pinned on gen_rf's three
    depths, this file feeds the whole-workload run (bench.py --workload c5)."""
    base = build_ctx(['Ca'])
    dbase = dump_inputs(base)
    Ns = base.atmos.Nspace
    out = {'tempPert': np.float64(50.0), 'Nspace': np.int32(Ns)}
    t0 = time.time()
    for k in range(Ns):
        for sgn, tag in ((+1, 'p'), (-1, 'm')):
            ctx = build_ctx(['Ca'], temp_pert=(k, sgn * 25.0))
            dp = dump_inputs(ctx)
            for key, v in dp.items():
                b = dbase[key]
                if v.dtype.kind in 'USib':
                    assert np.array_equal(v, b), key
                    continue
                if key.endswith('_n0') or np.array_equal(v, b):
                    continue
                if key == 'height':
                    assert np.array_equal(np.diff(v), np.diff(b)), 'height diff changed'
                    continue
                diff = (v != b)
                where_k = np.zeros_like(diff)
                where_k[..., k] = True
                assert not np.any(diff & ~where_k), 'non-local change in %s' % key
                out['k%d%s_%s' % (k, tag, key)] = v[..., k].copy()
        print('rf inputs: depth %d / %d  (%.0f s)' % (k + 1, Ns, time.time() - t0), flush=True)
    save(out_name, out)


def _delta_encode(dp, dbase, k):
    """gen_rf_inputs' delta encoding of one perturbed run: {key: v[..., k]} for every input array that differs from the base
    column's, asserting that it differs at depth k only"""
    out = {}
    for key, v in dp.items():
        b = dbase[key]
        if v.dtype.kind in 'USib':
            assert np.array_equal(v, b), key
            continue
        if key.endswith('_n0') or np.array_equal(v, b):
            continue
        if key == 'height':
            assert np.array_equal(np.diff(v), np.diff(b)), 'height diff changed'
            continue
        diff = (v != b)
        where_k = np.zeros_like(diff)
        where_k[..., k] = True
        assert not np.any(diff & ~where_k), 'non-local change in %s' % key
        out[key] = v[..., k].copy()
    return out


_RF_WORKER = {}


def _rf_worker_init(dbase, base_n, inputs_path):
    _RF_WORKER.update(dbase=dbase, base_n=base_n, inputs=dict(np.load(inputs_path)))


def _rf_run(job):
    """one perturbed run of gen_rf_outputs (in a worker process): -> (pre, {result key: array})"""
    k, sgn, tag = job
    w = _RF_WORKER
    pre = 'k%d%s_' % (k, tag)
    ctx = build_ctx(['Ca'], temp_pert=(k, sgn * 25.0), start_pops={'Ca': w['base_n']})
    # the inputs of this run are, bit for bit, the ones rf_ca_inputs.npz holds for it
    mine = _delta_encode(dump_inputs(ctx), w['dbase'], k)
    theirs = {key[len(pre):]: v for key, v in w['inputs'].items() if key.startswith(pre)}
    assert set(mine) == set(theirs), (pre, sorted(set(mine) ^ set(theirs)))
    for key, v in mine.items():
        assert np.array_equal(v, theirs[key]), pre + key
    t = {}
    n = run_mali(ctx, t, snap_iters=())
    return pre, {'I': ctx.I[:, -1:].copy(), 'n': ctx.activeAtoms[0].n.copy(), 'niter': np.int32(n),
                 'traj_dJ': t['traj_dJ'], 'traj_dPops': t['traj_dPops']}


def gen_rf_outputs(out_name='rf_ca_outputs.npz', workers=16):
    """the reference's converged OUTPUTS of all 2 x Nspace perturbed runs of response_fn.py:23-57 (the inputs are
    rf_ca_inputs.npz's; every run's delta-encoded inputs are asserted equal to that file's bit for bit), warm started like
    gen_rf from the reference's own converged base populations.  Per run: I at mu index -1 only (what the response function
    uses; all rays would put the file over the size limit of a committed file), n, the iteration count and the dJ / dPops
    trajectories; base_I (all rays), base_n, base_niter.  A pool of at most `workers` processes (about 10 s per run).
    Even so the plain arrays compress to 1.15 MB: every run's I and n are stored as their float64 bit patterns XOR those of the
    base column's (base_I[:, -1:], base_n; uint64, lossless), whose leading bits they share -- 0.93 MB.  Decode with
    (x ^ base.view(np.uint64)).view(np.float64)."""
    import multiprocessing as mp
    base = build_ctx(['Ca'])
    dbase = dump_inputs(base)
    tmp = {}
    run_mali(base, tmp, snap_iters=(), log='rf_base')
    base_n = base.eqPops['Ca'].n.copy()
    out = {'base_I': base.I.copy(), 'base_n': base.activeAtoms[0].n.copy(), 'base_niter': tmp['n_iter']}
    Ns = base.atmos.Nspace
    jobs = [(k, sgn, tag) for k in range(Ns) for sgn, tag in ((+1, 'p'), (-1, 'm'))]
    t0 = time.time()
    nproc = max(1, min(workers, len(os.sched_getaffinity(0))))
    with mp.get_context('spawn').Pool(nproc, _rf_worker_init, (dbase, base_n, os.path.join(HERE, 'rf_ca_inputs.npz'))) as pool:
        for q, (pre, res) in enumerate(pool.imap(_rf_run, jobs)):
            res['I'] = res['I'].view(np.uint64) ^ out['base_I'][:, -1:].copy().view(np.uint64)
            res['n'] = res['n'].view(np.uint64) ^ out['base_n'].view(np.uint64)
            for key, v in res.items():
                out[pre + key] = v
            print('rf outputs: %s%d iterations  (%d / %d, %.0f s)' % (pre, res['niter'], q + 1, len(jobs), time.time() - t0), flush=True)
    save(out_name, out)


def _atom_core(model, d, pre):
    """what the library's set-up chain reads of one AtomicModel (lightspinner_amd/atomdata.py from_fixture,
    tests/helpers.py build_data_fakes): weight, abundance, levels, each line's damping data, the collision tables"""
    import collisional_rates as cr
    from atomic_model import VdwUnsold
    tab = model.atomicTable
    d[pre + 'weight'] = np.float64(tab[model.name].weight)
    d[pre + 'abundance'] = np.float64(tab[model.name].abundance)
    d[pre + 'lev_E_SI'] = np.array([l.E_SI for l in model.levels])
    d[pre + 'lev_g'] = np.array([l.g for l in model.levels])
    d[pre + 'lev_stage'] = np.array([l.stage for l in model.levels], dtype=np.int32)
    L = model.lines
    d[pre + 'line_i'] = np.array([l.i for l in L], dtype=np.int32)
    d[pre + 'line_j'] = np.array([l.j for l in L], dtype=np.int32)
    for key in ('gRad', 'stark'):
        d[pre + 'line_' + key] = np.array([getattr(l, key) for l in L], dtype=np.float64)
    d[pre + 'line_vdw_unsold'] = np.array([1 if isinstance(l.vdw, VdwUnsold) else 0 for l in L], dtype=np.int32)
    d[pre + 'line_vdw_vals'] = np.array([list(l.vdw.vals)[:2] for l in L], dtype=np.float64).reshape(len(L), 2)
    kinds = {cr.Omega: 0, cr.CI: 1, cr.CE: 2}
    K = model.collisions
    d[pre + 'col_kind'] = np.array([kinds[type(c)] for c in K], dtype=np.int32)
    d[pre + 'col_i'] = np.array([c.i for c in K], dtype=np.int32)
    d[pre + 'col_j'] = np.array([c.j for c in K], dtype=np.int32)
    nt = max(len(c.temperature) for c in K)
    d[pre + 'col_nT'] = np.array([len(c.temperature) for c in K], dtype=np.int32)
    T = np.zeros((len(K), nt)); R = np.zeros((len(K), nt))
    for q, c in enumerate(K):
        T[q, :len(c.temperature)] = c.temperature
        R[q, :len(c.rates)] = c.rates
    d[pre + 'col_T'] = T
    d[pre + 'col_rates'] = R


def _atom_data(model, d, pre, fresh):
    """numeric content of one AtomicModel (rh_atoms.py data, atomic_model.py derived constants) as flat arrays.
    `fresh` is an identical model on which compute_wavelength_grid has NOT run: its transitions still carry the local
    wavelength grids the merge starts from (atomic_model.py:347-380, 585-597, 645-660)."""
    from atomic_model import HydrogenicContinuum
    core = {}
    _atom_core(model, core, pre)
    for key in ('weight', 'abundance', 'lev_E_SI', 'lev_g', 'lev_stage', 'line_i', 'line_j'):     # (the file's key order)
        d[pre + key] = core[pre + key]
    L = model.lines
    for key in ('f', 'gRad', 'stark', 'lambda0', 'Aji', 'Bji', 'Bij', 'qCore', 'qWing'):
        d[pre + 'line_' + key] = np.array([getattr(l, key) for l in L], dtype=np.float64)
    d[pre + 'line_NlambdaGen'] = np.array([l.NlambdaGen for l in L], dtype=np.int32)
    d[pre + 'line_vdw_unsold'], d[pre + 'line_vdw_vals'] = core[pre + 'line_vdw_unsold'], core[pre + 'line_vdw_vals']
    d[pre + 'line_vdw_cross'] = np.array([getattr(l.vdw, 'cross', 0.0) for l in L], dtype=np.float64)
    for q, l in enumerate(fresh.lines):
        d[pre + 'line%d_grid0' % q] = np.array(l.wavelength)
    Cn = model.continua
    d[pre + 'cont_i'] = np.array([c.i for c in Cn], dtype=np.int32)
    d[pre + 'cont_j'] = np.array([c.j for c in Cn], dtype=np.int32)
    d[pre + 'cont_edge'] = np.array([c.lambdaEdge for c in Cn])
    d[pre + 'cont_minLambda'] = np.array([c.minLambda for c in Cn])
    d[pre + 'cont_hydrogenic'] = np.array([1 if isinstance(c, HydrogenicContinuum) else 0 for c in Cn], dtype=np.int32)
    d[pre + 'cont_alpha0'] = np.array([getattr(c, 'alpha0', 0.0) for c in Cn])
    for q, c in enumerate(fresh.continua):
        d[pre + 'cont%d_grid0' % q] = np.array(c.wavelength)
        d[pre + 'cont%d_alpha_grid0' % q] = np.array(c.alpha)
    for q, c in enumerate(Cn):
        d[pre + 'cont%d_alpha' % q] = np.array(c.alpha)             # on the merged grid (compute_alpha)
        d[pre + 'cont%d_wavelength' % q] = np.array(c.wavelength)
    for key in ('col_kind', 'col_i', 'col_j', 'col_nT', 'col_T', 'col_rates'):
        d[pre + key] = core[pre + key]


def gen_setup():
    """Set-up chain that defines the hot-path inputs: atomic data of the two models of
    test.py, the wavelength-grid merge (atomic_set.py:377-455) and, for FALC and for a perturbed atmosphere, the
    reference's v_broad (atomic_model.py:66-69), damping (:491-502: radiative + Unsold van der Waals :166-198 + Stark
    :300-345), collisional rates (collisional_rates.py:10-96 with scipy's cubic interp1d) and LTE populations
    (atomic_set.py:105-145)."""
    d = {}
    variants = []
    k = np.arange(82)
    for tag, dT, fv, fne in (('atm0', None, 1.0, 1.0),
                             ('atm1', 600.0 * np.sin(2 * np.pi * k / 30.0) * np.exp(-((k - 40.0) / 30.0) ** 2) + 150.0, 1.7, 0.6)):
        ac = Falc82()
        ac.quadrature(5)
        if dT is not None:
            ac.temperature[:] = ac.temperature + dT * ac.temperature.unit
            ac.vturb[:] = ac.vturb * fv
            ac.ne[:] = ac.ne * fne
        atmos = ac.convert_scales()
        aSet = RadiativeSet([CaII_atom(), H_6_atom()])
        aSet.set_active('Ca', 'H')
        fresh = {m.name: m for m in RadiativeSet([CaII_atom(), H_6_atom()]).atoms}
        spect = aSet.compute_wavelength_grid()
        eqPops = aSet.compute_eq_pops(atmos)
        background = Background(atmos, spect)
        ctx = Context(atmos, spect, eqPops, background)
        for key in ('temperature', 'ne', 'vturb', 'nHTot'):
            d['%s_%s' % (tag, key)] = np.array(getattr(atmos, key), dtype=np.float64)
        d['%s_hGround' % tag] = np.array(eqPops['H'].n[0])
        for a, atom in enumerate(ctx.activeAtoms):
            pre = '%s_a%d_' % (tag, a)
            atom.compute_collisions()
            d[pre + 'vBroad'] = np.array(atom.vBroad)
            d[pre + 'nStar'] = np.array(atom.nStar)
            d[pre + 'nTotal'] = np.array(atom.nTotal)
            d[pre + 'C'] = np.array(atom.C)
            lines = [t for t in atom.trans if t.isLine]
            aD, Qe = [], []
            for t in lines:
                a_, q_ = t.transModel.damping(atmos, atom.vBroad, atom.hPops.n[0])
                aD.append(a_); Qe.append(q_)
            d[pre + 'aDamp'] = np.array(aD)
            d[pre + 'Qelast'] = np.array(Qe)
        if tag == 'atm0':
            d['atom_names'] = np.array([a.atomicModel.name for a in ctx.activeAtoms])
            tabH, tabHe = ctx.activeAtoms[0].atomicTable['H'], ctx.activeAtoms[0].atomicTable['He']
            d['weight_H'] = np.float64(tabH.weight); d['weight_He'] = np.float64(tabHe.weight)
            d['abundance_He'] = np.float64(tabHe.abundance)
            for a, atom in enumerate(ctx.activeAtoms):
                _atom_data(atom.atomicModel, d, 'm%d_' % a, fresh[atom.atomicModel.name])
            # the merge itself: inputs are the *_grid0 arrays + continuum edges + lambdaReference; outputs:
            d['grid_lambdaReference'] = np.float64(500.0)
            d['grid_wavelength'] = np.array(spect.wavelength)
            # spect.transitions order = iteration order of a Python set of models: record which (atom, kind, index) each is
            order = []
            for t in spect.transitions:
                a = [x.atomicModel for x in ctx.activeAtoms].index(t.atom)
                m = ctx.activeAtoms[a].atomicModel
                isline = isinstance(t, AtomicLine)
                q = [id(x) for x in (m.lines if isline else m.continua)].index(id(t))
                order.append((a, 1 if isline else 0, q))
            d['grid_trans_order'] = np.array(order, dtype=np.int32)
            d['grid_blueIdx'] = np.array([int(b) for b in spect.blueIdx], dtype=np.int32)
            d['grid_Nlambda'] = np.array([t.wavelength.shape[0] for t in spect.transitions], dtype=np.int32)
            act = np.zeros((len(spect.transitions), spect.wavelength.shape[0]), dtype=np.bool_)
            ids = [id(t) for t in spect.transitions]
            for la, sset in enumerate(spect.activeSet):
                for t in sset:
                    act[ids.index(id(t)), la] = True
            d['grid_active'] = act
    save('setup_falc.npz', d)


SETUP_ATOMS = (('H', H_6_atom), ('C', C_atom), ('MG', MgII_atom), ('CA', CaII_atom), ('FE', Fe_simple_atom))   # falc_all's order


def edge_atmosphere(knots, Ns=82, seed=20261016):
    """temperature, ne, vturb of the `edge` column: below 1000 K, 1000-3000 K, every knot of every collision table exactly,
    a few knots x (1 -+ 1e-12) and one ulp either side, values between the knots, above 30 000 K and up to 1e6 K; ne log-spaced
    over 1e12 ... 1e23 m^-3 and vturb over 0 ... 3e4 m/s, both shuffled against the temperatures"""
    rng = np.random.default_rng(seed)
    k = np.array(sorted(knots), dtype=np.float64)
    T = [400.0, 600.0, 800.0, 999.9, 1200.0, 1700.0, 2200.0, 2700.0, 2999.0]
    T += list(k)
    for x in (k[0], k[1], k[4], k[7], k[-1]):
        T += [x * (1.0 - 1e-12), x * (1.0 + 1e-12)]
    for x in (k[1], k[-1]):
        T += [np.nextafter(x, 0.0), np.nextafter(x, np.inf)]
    for lo, hi in zip(k[:-1], k[1:]):
        T += list(lo + (hi - lo) * np.array([0.13, 0.5, 0.87]))
    T += [1.2e5, 1.5e5, 2e5, 3e5, 5e5, 7e5, 1e6]
    T += list(np.exp(rng.uniform(np.log(400.0), np.log(1e6), Ns - len(T))))
    T = np.array(T)
    assert T.shape == (Ns,)
    ne = rng.permutation(np.logspace(12.0, 23.0, Ns))
    vturb = rng.permutation(np.linspace(0.0, 3e4, Ns))
    return T, ne, vturb


def _setup_chain(models, atmos):
    """the reference's set-up chain at one atmosphere, called method by method (at the edge temperatures neither
    Atmosphere.convert_scales nor Background can be built): compute_eq_pops (atomic_set.py:361-375: LTE with Debye
    lowering), v_broad (atomic_model.py:66-69), each line's damping (:491-502) with H's ground-level population, each
    collision's compute_rates and the clamp of compute_collisions (rh_method.py:474-487).  models in falc_all's order"""
    eqPops = RadiativeSet(models).compute_eq_pops(atmos)
    hGround = np.array(eqPops['H'].n[0])
    out = {'hGround': hGround}
    for a, m in enumerate(models):
        st = eqPops[m.name]
        vB = np.array(m.v_broad(atmos))
        Nl = len(m.levels)
        C = np.zeros((Nl, Nl, atmos.Nspace))
        for col in m.collisions:
            col.compute_rates(atmos, st.nStar, C)
        C[C < 0.0] = 0.0
        out['a%d_vBroad' % a] = vB
        out['a%d_nStar' % a] = np.array(st.nStar)
        out['a%d_nTotal' % a] = np.array(st.nTotal)
        out['a%d_C' % a] = C
        out['a%d_aDamp' % a] = np.array([l.damping(atmos, vB, hGround)[0] for l in m.lines])   # model line order
    return out


def gen_setup_atoms():
    """Atomic data of all five of the reference's model atoms (the keys lightspinner_amd/atomdata.py from_fixture and
    tests/helpers.py build_data_fakes read) and the reference's set-up outputs for the 82-depth `edge` column
    (edge_atmosphere: FALC's nHTot, temperatures from 400 K to 1e6 K).  The same code run at FALC must reproduce
    falc_all.npz's vBroad, nStar, C and aDamp bit for bit; FALC's outputs are not stored a second time."""
    ref = dict(np.load(os.path.join(HERE, 'falc_all.npz')))
    models = [ctor() for _, ctor in SETUP_ATOMS]
    RadiativeSet(models)                                         # gives every model its atomic table
    assert [m.name for m in models] == [str(x) for x in ref['atom_names']]
    d = {'atom_names': np.array([m.name for m in models])}
    for a, m in enumerate(models):
        _atom_core(m, d, 'm%d_' % a)
    tab = models[0].atomicTable
    d['weight_H'], d['weight_He'] = np.float64(tab['H'].weight), np.float64(tab['He'].weight)
    d['abundance_He'] = np.float64(tab['He'].abundance)

    def falc():
        ac = Falc82()
        ac.quadrature(5)
        atmos = ac.convert_scales()
        atmos.nondimensionalise()
        return atmos
    # FALC: bit for bit what falc_all.npz holds (its Context made the same calls)
    atmos = falc()
    assert np.array_equal(np.asarray(atmos.temperature), ref['temperature']) and np.array_equal(np.asarray(atmos.ne), ref['ne'])
    out = _setup_chain(models, atmos)
    assert np.array_equal(out['hGround'], ref['hGround'])
    for a, m in enumerate(models):
        for key in ('vBroad', 'nStar', 'nTotal', 'C'):
            assert np.array_equal(out['a%d_%s' % (a, key)], ref['a%d_%s' % (a, key)]), (m.name, key)
        lines = [kr for kr in range(ref['t_atom'].shape[0]) if ref['t_atom'][kr] == a and ref['t_isline'][kr]]
        assert [(int(ref['t_i'][kr]), int(ref['t_j'][kr])) for kr in lines] == [(l.i, l.j) for l in m.lines], m.name
        for q, kr in enumerate(lines):
            assert np.array_equal(out['a%d_aDamp' % a][q], ref['t%d_aDamp' % kr]), (m.name, kr)
    knots = {float(x) for m in models for c in m.collisions for x in c.temperature}
    T, ne, vturb = edge_atmosphere(knots)
    atmos = falc()
    atmos.temperature, atmos.ne, atmos.vturb = T, ne, vturb
    out = _setup_chain(models, atmos)
    for key in ('temperature', 'ne', 'vturb', 'nHTot'):
        d['edge_' + key] = np.array(getattr(atmos, key), dtype=np.float64)
    for key, v in out.items():
        d['edge_' + key] = v
    save('setup_atoms.npz', d)

def gen_live_ref(n_iter=6):
    """What tests/test_reference_live.py compares with: the reference's FALC CaII Context (test.py's set-up) through six MALI
    iterations, and the merged wavelength grid of RadiativeSet([CaII, H_6]) with Ca and H active.  Everything falc_ca.npz and
    setup_falc.npz already hold (vBroad, per transition Nblue / active / aDamp / phi / wphi, iterations 1-5, C, the grid, its
    blueIdx, the transitions' grids and alpha, the active sets) is checked here to be bit for bit what this run computes; the
    file keeps only the rest: each line's wlambda, iteration 6 (dJ, J, I) and its statistical equilibrium (dPops, n)."""
    ca = dict(np.load(os.path.join(HERE, 'falc_ca.npz')))
    st = dict(np.load(os.path.join(HERE, 'setup_falc.npz')))
    d = {}
    ctx = build_ctx(['Ca'])
    atom = ctx.activeAtoms[0]
    assert np.array_equal(atom.vBroad, ca['a0_vBroad'])
    for kr, t in enumerate(atom.trans):
        assert t.Nblue == ca['t_Nblue'][kr] and np.array_equal(t.active, ca['t_active'][kr])
        if t.isLine:
            aDamp = t.transModel.damping(ctx.atmos, atom.vBroad, atom.hPops.n[0])[0]
            phi = ca['t%d_phi' % kr]
            assert np.array_equal(aDamp, ca['t%d_aDamp' % kr]) and np.array_equal(t.wphi, ca['t%d_wphi' % kr])
            assert np.array_equal(t.phi, phi if phi.ndim == 4 else np.broadcast_to(phi[:, None, None, :], t.phi.shape))
            d['t%d_wlambda' % kr] = np.array(t.wlambda())
    for it in range(1, n_iter + 1):
        dJ = ctx.formal_sol_gamma_matrices()
        assert np.array_equal(atom.C, ca['a0_C'])
        if it < n_iter:
            assert dJ == ca['fs%d_dJ' % it] and np.array_equal(ctx.J, ca['fs%d_J' % it]) and np.array_equal(ctx.I, ca['fs%d_I' % it])
        else:
            d['fs%d_dJ' % it], d['fs%d_J' % it], d['fs%d_I' % it] = np.float64(dJ), ctx.J.copy(), ctx.I.copy()
        if it > 3:
            dPops = ctx.stat_equil()
            if it < n_iter:
                assert dPops == ca['se%d_dPops' % it] and np.array_equal(ctx.eqPops['Ca'].n, ca['se%d_n_a0' % it])
            else:
                d['se%d_dPops' % it], d['se%d_n' % it] = np.float64(dPops), np.array(ctx.eqPops['Ca'].n)
    aSet = RadiativeSet([CaII_atom(), H_6_atom()])
    aSet.set_active('Ca', 'H')
    spect = aSet.compute_wavelength_grid()
    names = [str(x) for x in st['atom_names']]
    assert [m.name for m in spect.models] == names
    assert np.array_equal(spect.wavelength, st['grid_wavelength']) and list(spect.blueIdx) == list(st['grid_blueIdx'])
    for k, (t, (a, il, q)) in enumerate(zip(spect.transitions, st['grid_trans_order'])):
        pre = 'm%d_%s_' % (a, 'line' if il else 'cont')
        assert (t.atom.name, t.i, t.j) == (names[a], st[pre + 'i'][q], st[pre + 'j'][q])
        assert np.array_equal(t.wavelength, st['grid_wavelength'][st['grid_blueIdx'][k]:][:st['grid_Nlambda'][k]])
        assert isinstance(t, AtomicLine) == bool(il) and (il or np.array_equal(t.alpha, st['m%d_cont%d_alpha' % (a, q)]))
    for la, s in enumerate(spect.activeSet):
        assert [spect.transitions.index(t) for t in s] == list(np.nonzero(st['grid_active'][:, la])[0])
    save('live_ref.npz', d)


if __name__ == '__main__':
    what = sys.argv[1:] or ['all']
    if 'all' in what:
        what = ['units', 'falc_ca', 'falc_cah', 'falc_ca_vlos', 'falc_c', 'falc_fe', 'falc_mg', 'falc_all', 'rf']
    for w in what:
        t0 = time.time()
        {'units': gen_units, 'falc_ca': gen_falc_ca, 'falc_cah': gen_falc_cah,
         'falc_ca_vlos': gen_falc_ca_vlos, 'rf': gen_rf, 'falc_c': lambda: gen_falc_multilevel('c'),
         'falc_fe': lambda: gen_falc_multilevel('fe'), 'falc_mg': lambda: gen_falc_multilevel('mg'), 'falc_all': gen_falc_all, 'rf_inputs': gen_rf_inputs, 'rf_outputs': gen_rf_outputs, 'setup': gen_setup,
         'live_ref': gen_live_ref, 'setup_atoms': gen_setup_atoms}[w]()
        print('%s done in %.1fs' % (w, time.time() - t0), flush=True)
