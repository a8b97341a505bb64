"""LTE populations of an atmosphere's atoms on the GPU: the reference's RadiativeSet.compute_eq_pops (atomic_set.py:361-375) over
lte_pops(debye=True) (:105-145), through include/lsx_hip_eqpops.h.

    eqPops = compute_eq_pops(models, atmos)            # eqPops['H'].n[0], eqPops['Ca'].nStar / .nTotal / .pops
    ctx = rh_method.Context(atmos, spect, eqPops, background)

For many columns use Engine.eq_pops (problem.py), which takes [ncol][Nspace] arrays and any atoms, active in the engine or not.
"""
import ctypes as C

import numpy as np

from . import _capi


def atoms_to_c(atoms, abundances):
    """atoms: objects with .E_SI, .g, .stage per level -> (lsx_eq_atom array, [Nlevel per atom], keepalive)"""
    atoms = list(atoms)
    ab = [float(x) for x in np.asarray(abundances, dtype=np.float64).reshape(-1)]
    if len(ab) != len(atoms):
        raise ValueError('%d abundances for %d atoms' % (len(ab), len(atoms)))
    arr = (_capi.LsxEqAtom * max(1, len(atoms)))()
    keep, nlev = [], []
    for a, atom in enumerate(atoms):
        E, g, st = np.asarray(atom.E_SI, dtype=np.float64), np.asarray(atom.g, dtype=np.float64), np.asarray(atom.stage)
        nl = int(g.shape[0])
        if E.shape != (nl,) or st.shape != (nl,):
            raise ValueError('atom %d: E_SI, g and stage differ in length' % a)
        lev = (_capi.LsxLevel * max(1, nl))()
        for q in range(nl):
            lev[q] = _capi.LsxLevel(float(E[q]), float(g[q]), int(st[q]), 0)
        arr[a] = _capi.LsxEqAtom(nl, 0, lev, ab[a])
        keep.append(lev)
        nlev.append(nl)
    return arr, nlev, keep


class EqPops:
    """What Engine.eq_pops returns: .nStar_flat [ncol][sum Nlevel][Nspace], .nStar (per atom, views [ncol][Nlevel][Nspace]) and
    .nTotal [ncol][natoms][Nspace] (or None)"""

    def __init__(self, nStar_flat, nTotal, nlev):
        self.nStar_flat, self.nTotal = nStar_flat, nTotal
        off = np.concatenate([[0], np.cumsum(nlev)]).astype(int)
        self.nStar = [nStar_flat[:, off[a]:off[a + 1]] for a in range(len(nlev))]


class AtomState:
    """One atom of an EqPopsTable: .model, .nStar [Nlevel][Nspace], .nTotal [Nspace], .pops (None until a Context or the caller
    sets it) and .n, the populations in force: pops where set, else nStar."""

    def __init__(self, model, nStar, nTotal, pops=None):
        self.model, self.nStar, self.nTotal, self.pops = model, nStar, nTotal, pops

    @property
    def name(self):
        return self.model.name

    @property
    def n(self):
        return self.nStar if self.pops is None else self.pops


def _key(name):
    return str(name).upper().strip()


class EqPopsTable:
    """The atoms' states, indexable by element name in any case ('H', 'Ca', 'CA')."""

    def __init__(self, atmos, atomicTable, atoms):
        self.atmos, self.atomicTable, self.atoms = atmos, atomicTable, list(atoms)
        self._index = {_key(a.name): q for q, a in enumerate(self.atoms)}

    def __contains__(self, name):
        return _key(name) in self._index

    def __len__(self):
        return len(self.atoms)

    def __getitem__(self, name):
        return self.atoms[self._index[_key(name)]]

    def __iter__(self):
        return iter(self.atoms)


def compute_eq_pops(models, atmos, device=0, lib=None):
    """Drop-in for RadiativeSet.compute_eq_pops on Lightspinner-shaped objects.  models: every atom of the set (each with .name,
    .levels[].E_SI / .g / .stage and .atomicTable[name].abundance / .weight); atmos carries temperature, ne and nHTot in SI (it is
    nondimensionalised for the call where it has the method and is dimensioned, as atomic_set.py:362-365 does, and like there it
    is left so: the reference's :374 names dimensionalise without calling it).
    -> EqPopsTable, atoms in order of atomic weight."""
    from .background import _carrier_problem
    from .problem import Engine
    models = list(models)
    if not models:
        raise ValueError('compute_eq_pops: no atoms')
    table = models[0].atomicTable
    models = sorted(models, key=lambda m: float(table[m.name].weight))
    if getattr(atmos, 'dimensioned', False) and hasattr(atmos, 'nondimensionalise'):
        atmos.nondimensionalise()
    T, ne, nH = (np.asarray(getattr(atmos, k), dtype=np.float64) for k in ('temperature', 'ne', 'nHTot'))

    class _Levels:
        def __init__(self, m):
            self.E_SI = [l.E_SI for l in m.levels]
            self.g = [l.g for l in m.levels]
            self.stage = [l.stage for l in m.levels]
    eng = Engine(_carrier_problem(T.shape[0]), 1, device=device, lib=lib)
    try:
        r = eng.eq_pops([_Levels(m) for m in models], [table[m.name].abundance for m in models], T, ne, nH)
    finally:
        eng.close()
    return EqPopsTable(atmos, table, [AtomState(m, np.array(r.nStar[a][0]), np.array(r.nTotal[0, a])) for a, m in enumerate(models)])
