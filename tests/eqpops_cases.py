"""What the LTE-population tests share (tests/test_eqpops_host.py, tests/test_eqpops.py): a numpy restatement of the reference's
lte_pops(debye=True) (atomic_set.py:105-145), the cases read from committed fixtures, the CPU build of lsx_eqpops_dev.h
(liblsx_eqpops_host.so, `make eqpopshost`) and the bar.

The bar is the set-up chain's (tests/setup_cases.py, nstar_bar), with no new number: entry by entry and relative to the entry,
    EPS (16 + 8 |x_i| + 8 max_l |x_l|),   x_i = dE_i / kT,
which counts the roundings of the argument of exp (4 EPS on the library's side, 4 on the reference's, turned into an absolute error
|x_i| 8 EPS by exp) for the level itself and for the largest term of the sum behind nStar_0.  At the edge temperature of 400 K,
|x| reaches 4e2 (hydrogen's 13.6 eV over 0.034 eV) and the bar 1.5e-12: it grows with max_i |dE_i / kT| u exactly as the rounding
of the exponent's argument does, so no separate edge bar is needed; a bar above 1e-9 anywhere fails the check as vacuous.  Entries
the reference holds at 0 (underflow) must be 0."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from conftest import ROOT, golden

import setup_cases as sc
from lightspinner_amd import _capi, constants as K
from lightspinner_amd.eqpops import EqPops, atoms_to_c

CSRC = os.path.join(ROOT, 'lightspinner_amd', 'csrc')
VACUOUS = 1e-9
EINVAL = 1


class Atom:
    """the levels of one atom: what Engine.eq_pops reads of an atomdata.AtomData"""

    def __init__(self, E_SI, g, stage, name=''):
        self.E_SI, self.g, self.stage, self.name = np.asarray(E_SI, dtype=np.float64), np.asarray(g, dtype=np.float64), np.asarray(stage), name


def lte_numpy(atom, T, ne, nTotal):
    """atomic_set.py:105-145 with debye=True, operation by operation, on arrays of any shape -> [Nlevel] + T.shape"""
    T, ne, nTotal = (np.asarray(a, dtype=np.float64) for a in (T, ne, nTotal))
    Nl = len(atom.g)
    c1 = (K.HPlanck / (2.0 * np.pi * K.MElectron)) * (K.HPlanck / K.KBoltzmann)
    c2 = np.sqrt(8.0 * np.pi / K.KBoltzmann) * (K.QElectron**2 / (4.0 * np.pi * K.Epsilon0))**1.5
    nDebye = np.zeros(Nl)
    for i in range(1, Nl):
        Z = int(atom.stage[i])
        for _ in range(1, int(atom.stage[i]) - int(atom.stage[0]) + 1):
            nDebye[i] += Z
            Z += 1
    dEion = c2 * np.sqrt(ne / T)
    cNe_T = 0.5 * ne * (c1 / T)**1.5
    total = np.ones(T.shape)
    nStar = np.zeros((Nl,) + T.shape)
    with np.errstate(over='ignore', under='ignore', divide='ignore'):
        for i in range(1, Nl):
            dE = atom.E_SI[i] - atom.E_SI[0]
            gi0 = atom.g[i] / atom.g[0]
            dZ = int(atom.stage[i]) - int(atom.stage[0])
            dE_kT = (dE - nDebye[i] * dEion) / (K.KBoltzmann * T)
            nStar[i] = gi0 * np.exp(-dE_kT)
            nStar[i] /= cNe_T**dZ
            total += nStar[i]
        nStar[0] = nTotal / total
        for i in range(1, Nl):
            nStar[i] *= nStar[0]
    return nStar


def bar(atom, T):
    """the set-up chain's bar for nStar, [Nlevel] + T.shape; vacuous above 1e-9"""
    T = np.asarray(T, dtype=np.float64)
    b = sc.nstar_bar(atom.E_SI, T.reshape(-1)).reshape((len(atom.g),) + T.shape)
    assert np.all(b <= VACUOUS), ('vacuous bar', float(b.max()))
    return b


def check(led, what, got, ref, atom, T, factor=1.0, mask=None, rows=slice(None)):
    """got, ref [ncol][Nlevel][Ns] (rows: the levels they hold), T [ncol][Ns]; mask [ncol][Ns]: the points the reference covers"""
    got, ref = np.asarray(got), np.asarray(ref)
    b = np.moveaxis(bar(atom, T), 0, 1)[:, rows] * factor
    if mask is not None:
        m = np.broadcast_to(np.asarray(mask, dtype=bool)[:, None, :], got.shape)
        got, ref, b = got[m], ref[m], b[m]
    assert np.all(np.isfinite(got)), what
    led.check(what, got, ref, b)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _npz(name):
    return dict(np.load(golden(name)))


def fixture_atoms(d):
    """-> ([Atom], [abundance]) of a set-up fixture (setup_falc.npz: H, Ca; setup_atoms.npz: H, C, Mg, Ca, Fe)"""
    names = [str(x) for x in d['atom_names']]
    atoms = [Atom(d['m%d_lev_E_SI' % a], d['m%d_lev_g' % a], d['m%d_lev_stage' % a], names[a]) for a in range(len(names))]
    return atoms, [float(d['m%d_abundance' % a]) for a in range(len(names))]


class Case:
    """atoms, abundances, the atmosphere [ncol][Ns] and the reference's nStar per atom [ncol][Nlevel][Ns] (None: not recorded) with
    the mask of the points it covers; hGround [ncol][Ns] where the fixture holds it (atom 0 is hydrogen then)"""

    def __init__(self, name, atoms, ab, T, ne, nH, ref, mask=None, hGround=None):
        self.name, self.atoms, self.ab = name, atoms, ab
        self.T, self.ne, self.nH = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (T, ne, nH))
        self.ref, self.mask, self.hGround = ref, mask, hGround


def falc_cases():
    """hydrogen and calcium on the two atmospheres of setup_falc.npz"""
    d = _npz('setup_falc.npz')
    atoms, ab = fixture_atoms(d)
    out = []
    for q in (0, 1):
        p = 'atm%d_' % q
        out.append(Case('falc_atm%d' % q, atoms, ab, d[p + 'temperature'], d[p + 'ne'], d[p + 'nHTot'],
                        [d[p + 'a%d_nStar' % a][None] for a in range(2)], hGround=d[p + 'hGround'][None]))
    return out


def response_case():
    """H + Ca at the 164 points of the temperature response function (rf_ca_inputs.npz) as one [2][82] batch: row 0 holds T[k] + 25 K
    at EVERY depth k, row 1 T[k] - 25 K (the populations are pointwise in depth); the reference's hGround and Ca nStar at depth k of
    run k are the entries of column k"""
    d, r, f = _npz('setup_falc.npz'), _npz('rf_ca_inputs.npz'), _npz('falc_ca.npz')
    atoms, ab = fixture_atoms(d)
    Ns = int(r['Nspace'])
    T, hG, ca = np.empty((2, Ns)), np.empty((2, Ns)), np.empty((2, 6, Ns))
    for c, tag in enumerate('pm'):
        for k in range(Ns):
            T[c, k], hG[c, k], ca[c, :, k] = r['k%d%s_temperature' % (k, tag)], r['k%d%s_hGround' % (k, tag)], r['k%d%s_a0_nStar' % (k, tag)]
    assert np.allclose(T[0] - T[1], float(r['tempPert']), rtol=0, atol=1e-9)
    two = lambda a: np.stack([a, a])
    return Case('rf_164', atoms, ab, T, two(f['ne']), two(f['nHTot']), [None, ca], hGround=hG)


def five_atom_case():
    """the five atoms of setup_atoms.npz in one call: FALC (falc_all.npz) and the edge atmosphere (400 K ... 1e6 K, ne 1e12 ... 1e23)"""
    s, f = _npz('setup_atoms.npz'), _npz('falc_all.npz')
    atoms, ab = fixture_atoms(s)
    ref = [np.stack([f['a%d_nStar' % a], s['edge_a%d_nStar' % a]]) for a in range(5)]
    return Case('five_atoms', atoms, ab, np.stack([f['temperature'], s['edge_temperature']]), np.stack([f['ne'], s['edge_ne']]),
                np.stack([f['nHTot'], s['edge_nHTot']]), ref, hGround=np.stack([f['hGround'], s['edge_hGround']]))


def all_cases():
    return falc_cases() + [response_case(), five_atom_case()]


def check_case(led, case, r, factor=1.0):
    """r: an EqPops (device or host build) of the case, against the fixtures"""
    for a, atom in enumerate(case.atoms):
        assert np.array_equal(r.nTotal[:, a], case.ab[a] * case.nH), (case.name, atom.name, 'nTotal')
        if case.ref[a] is not None:
            check(led, 'nStar', r.nStar[a], case.ref[a], atom, case.T, factor, case.mask)
    if case.hGround is not None:
        check(led, 'hGround', r.nStar[0][:, :1], case.hGround[:, None], case.atoms[0], case.T, factor, rows=slice(0, 1))


def numpy_result(case):
    nT = np.stack([ab * case.nH for ab in case.ab], axis=1)
    ns = [np.moveaxis(lte_numpy(atom, case.T, case.ne, nT[:, a]), 0, 1) for a, atom in enumerate(case.atoms)]
    return EqPops(np.concatenate(ns, axis=1), nT, [len(a.g) for a in case.atoms])


# ---- made-up atoms ------------------------------------------------------------------------------------------------------------------
_EV = 1.60217733E-19


def toy_atoms():
    """{name: (Atom, abundance)}: one level; two levels; dZ = 0, 1, 2, 3 in one atom (numpy's integer-power cases and pow); 40 levels
    over three stages; zero abundance"""
    rng = np.random.default_rng(20261019)
    forty_stage = np.repeat([1, 2, 3], [25, 10, 5])
    return {
        'one': (Atom([0.0], [2.0], [0]), 1.0),
        'two': (Atom([0.0, 10.2 * _EV], [2.0, 8.0], [0, 0]), 1e-3),
        'stages': (Atom(np.array([0.0, 2.1, 7.6, 9.0, 22.0, 23.5, 61.0]) * _EV, [1.0, 3.0, 2.0, 4.0, 1.0, 5.0, 2.0], [0, 0, 1, 1, 2, 2, 3]), 4e-5),
        'forty': (Atom(np.sort(rng.uniform(0.0, 6.0, 40)) * _EV + 7.0 * _EV * (forty_stage - 1), rng.integers(1, 9, 40) * 2.0, forty_stage), 2e-6),
        'absent': (Atom([0.0, 3.0 * _EV, 8.0 * _EV], [2.0, 6.0, 1.0], [0, 0, 1]), 0.0),
    }


def toy_atmosphere(ncol=2, Ns=13):
    rng = np.random.default_rng(7)
    return (10 ** rng.uniform(np.log10(3000.0), 5.0, (ncol, Ns)), 10 ** rng.uniform(14.0, 22.0, (ncol, Ns)), 10 ** rng.uniform(15.0, 23.0, (ncol, Ns)))


# ---- the CPU build -------------------------------------------------------------------------------------------------------------------
class HostLib:
    """liblsx_eqpops_host.so: lsx_eqpops_dev.h compiled for the CPU (`make eqpopshost`)"""

    def __init__(self):
        subprocess.check_call(['make', '-s', '-C', CSRC, 'eqpopshost'])
        self.dll = d = C.CDLL(os.path.join(CSRC, 'liblsx_eqpops_host.so'))
        dp = C.POINTER(C.c_double)
        d.lsx_eqpops_host_error.restype = C.c_char_p
        d.lsx_eqpops_host.argtypes = [C.c_int32, C.c_int32, C.POINTER(_capi.LsxEqAtom), C.c_int32, dp, dp, dp, dp, dp]

    def error(self):
        return self.dll.lsx_eqpops_host_error().decode()

    def raw(self, Ns, natoms, carr, ncol, T, ne, nH, nStar, nTotal):
        opt = lambda a: None if a is None else _capi._ptr(a)
        return self.dll.lsx_eqpops_host(Ns, natoms, carr, ncol, opt(T), opt(ne), opt(nH), opt(nStar), opt(nTotal))

    def eq_pops(self, atoms, ab, T, ne, nH, want_nTotal=True):
        """-> (rc, EqPops)"""
        T, ne, nH = (_capi.f64(np.atleast_2d(np.asarray(a, dtype=np.float64))) for a in (T, ne, nH))
        ncol, Ns = T.shape
        carr, nlev, _keep = atoms_to_c(atoms, ab)
        nStar = np.full((ncol, sum(nlev), Ns), np.nan)
        nTotal = np.full((ncol, len(nlev), Ns), np.nan) if want_nTotal else None
        rc = self.raw(Ns, len(nlev), carr, ncol, T, ne, nH, nStar, nTotal)
        return rc, EqPops(nStar, nTotal, nlev)

    def of_case(self, case):
        rc, r = self.eq_pops(case.atoms, case.ab, case.T, case.ne, case.nH)
        assert rc == 0, self.error()
        return r
