"""Native set-up of columns: from an atmosphere to a ready context entirely through device entries of the HIP library, with no
numerics on the host and no input taken from the reference ("Native set-up of a column range").

    setup = NativeSetup(atomic_data, hydrogen, abundances, tables, logG=2.44)
    model = ColumnModel('column_mass', cmass, temperature, ne, nHTot, vturb)          # arrays [ncol][Nspace], SI
    eng.setup_columns(0, model, setup)
"""
from dataclasses import dataclass, replace
from typing import Optional, Sequence

import numpy as np

from . import _capi
from ._capi import f64
from .problem import ColumnBlock

PARAMETERS = ('temperature', 'vturb', 'vlos', 'ne', 'nHTot')
_CHUNK = 64         # columns per pass: the placeholder block of set_columns stays small


@dataclass
class ColumnModel:
    """Atmospheres of ncol columns on one depth scale.  scale: 'column_mass', 'geometric' or 'tau500'; arrays [ncol][Nspace] in SI
    (one column may be 1-D); vlos optional (None: no line-of-sight velocity)."""
    scale: str
    depth_scale: np.ndarray
    temperature: np.ndarray
    ne: np.ndarray
    nHTot: np.ndarray
    vturb: np.ndarray
    vlos: Optional[np.ndarray] = None

    FIELDS = ('depth_scale', 'temperature', 'ne', 'nHTot', 'vturb', 'vlos')

    @property
    def ncol(self):
        return int(np.atleast_2d(self.temperature).shape[0])

    def validated(self, Nspace):
        """-> a copy with every array float64 [ncol][Nspace]"""
        T = f64(np.atleast_2d(np.asarray(self.temperature, dtype=np.float64)))
        if T.ndim != 2 or T.shape[1] != Nspace:
            raise ValueError('ColumnModel: temperature must be [ncol][%d], got %s' % (Nspace, T.shape))
        out = {}
        for k in self.FIELDS:
            v = getattr(self, k)
            out[k] = None if v is None else f64(np.atleast_2d(np.asarray(v, dtype=np.float64)), T.shape)
        if any(out[k] is None for k in self.FIELDS[:-1]):
            raise ValueError('ColumnModel: only vlos may be None')
        return ColumnModel(self.scale, **out)

    def slice(self, c0, c1):
        return ColumnModel(self.scale, **{k: (None if getattr(self, k) is None else getattr(self, k)[c0:c1]) for k in self.FIELDS})

    def repeated(self, n):
        """column 0, n times"""
        return ColumnModel(self.scale, **{k: (None if getattr(self, k) is None else np.repeat(np.atleast_2d(getattr(self, k))[:1], n, axis=0))
                                           for k in self.FIELDS})


@dataclass
class NativeSetup:
    """What the native set-up needs besides the atmosphere: atomic_data (atomdata.AtomicData of the active atoms, in the problem's
    order), hydrogen (an atomdata.AtomData; only its levels are read), abundances (of the active atoms, relative to hydrogen),
    tables (background.EosTables) and logG (read for the geometric scale only)."""
    atomic_data: object
    hydrogen: object
    abundances: Sequence[float]
    tables: object
    logG: float = 2.44


def setup_columns(eng, col0, model, setup, start_n=None):
    """Engine.setup_columns: columns [col0, col0 + model.ncol) of `eng` from `model` through device entries only, in this order:
      1. set_columns with a placeholder block of the right shapes (the library checks pointers only; every field it uploads is
         overwritten below, the temperature is the real one; phi = wphi = None);
      2. convert_scales(install=True): the heights;
      3. background(install=True, read_back=False): chi, eta and the Thomson term;
      4. eq_pops for hydrogen and the active atoms: nHGround = hydrogen's LTE ground population, nTotal = abundance x nHTot;
      5. set_atmosphere(lte_pops=True): broadening, damping, profiles, collisional rates, LTE populations, n = nStar;
      6. set(LSX_N, start_n) for a warm start (start_n [NLtot][Nspace] for all columns, or [ncol][NLtot][Nspace])."""
    p = eng.problem
    m = model.validated(p.Nspace)
    nc = m.ncol
    if col0 < 0 or col0 + nc > eng.ncol:
        raise ValueError('setup_columns: columns [%d, %d) outside the engine\'s %d' % (col0, col0 + nc, eng.ncol))
    if len(setup.atomic_data.atoms) != p.Natoms or len(setup.abundances) != p.Natoms:
        raise ValueError('setup_columns: the set-up holds %d atoms and %d abundances, the problem %d atoms'
                         % (len(setup.atomic_data.atoms), len(setup.abundances), p.Natoms))
    vlos = m.vlos
    if vlos is not None and p.phi_compact:
        if np.any(vlos != 0.0):
            raise ValueError('setup_columns: a phi_compact problem takes no line-of-sight velocity')
        vlos = None
    if start_n is not None:
        start_n = np.broadcast_to(np.asarray(start_n, dtype=np.float64), (nc, p.NLtot, p.Nspace))
    if not eng._have_atomic_data:
        eng.set_atomic_data(setup.atomic_data)
    atoms = [setup.hydrogen] + list(setup.atomic_data.atoms)
    abund = [1.0] + [float(a) for a in setup.abundances]
    for a in range(0, nc, _CHUNK):
        b = min(nc, a + _CHUNK)
        nb, s = b - a, m.slice(a, b)
        ones = lambda *shape: np.ones((nb,) + shape)
        eng.set_columns(col0 + a, ColumnBlock(height=ones(p.Nspace), temperature=s.temperature, nStar=ones(p.NLtot, p.Nspace),
                                              nTotal=ones(p.Natoms, p.Nspace), n=ones(p.NLtot, p.Nspace), C=ones(p.NL2tot, p.Nspace),
                                              bg_chi=ones(p.Nspect, p.Nspace), bg_eta=ones(p.Nspect, p.Nspace),
                                              bg_sca=ones(*p.sca_shape()), phi=None, wphi=None))
        eng.convert_scales(setup.tables, s.scale, s.depth_scale, s.temperature, s.nHTot, ne=s.ne, logG=setup.logG, col0=col0 + a,
                           install=True, read_back=False)
        eng.background(setup.tables, s.temperature, s.nHTot, s.ne, col0=col0 + a, install=True, read_back=False)
        r = eng.eq_pops(atoms, abund, s.temperature, s.ne, s.nHTot)
        eng.set_atmosphere(col0 + a, s.temperature, s.ne, s.vturb, np.ascontiguousarray(r.nStar[0][:, 0]),
                           np.ascontiguousarray(r.nTotal[:, 1:]), vlos=None if vlos is None else vlos[a:b], lte_pops=True)
        if start_n is not None:
            eng.set(_capi.LSX_N, np.ascontiguousarray(start_n[a:b]), col0 + a)


def perturbed(model, parameter, amplitude, ks):
    """model: one column.  -> ColumnModel of 2 len(ks) columns: column 2i is the model with q[ks[i]] + amplitude / 2, column 2i + 1
    the one with q[ks[i]] - amplitude / 2 (q = the array `parameter` names): the job order of response.run_response_function"""
    out = model.repeated(2 * len(ks))
    q = getattr(out, parameter)
    if q is None:                                   # vlos of a model at rest
        q = np.zeros_like(out.temperature)
    q = np.array(q, dtype=np.float64)
    for i, k in enumerate(ks):
        q[2 * i, k] += amplitude / 2
        q[2 * i + 1, k] -= amplitude / 2
    return replace(out, **{parameter: q})
