"""The background of an atmosphere on the GPU: the reference's Background(atmos, spect) (background.py:15-53) -- the Wittmann
equation of state and the ATLAS-style continuous opacity of witt.py -- through include/lsx_hip_background.h.

    tables = EosTables.from_kurucz_xdr('pf_Kurucz.input', abund, amass, weight_per_H)
    bg = Background(atmos, spect, tables)                    # .chi, .eta, .sca shaped as the reference's
    ctx = rh_method.Context(atmos, spect, eqPops, bg)

For many columns, or to put the result straight into an engine without a copy through the host, use Engine.eos /
Engine.background (problem.py).  The library reads no file: the partition functions are handed over as arrays.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import f64, _ptr

# witt.py:44-49: what turns the table's ionisation energies (cm^-1) into eV
_HH, _CC, _EV = 6.62606957E-27, 2.99792458E10, 1.602176565E-12
NPARTIALS = 17
# order of witt.getBackgroundPartials(divide_by_u=True) (witt.py:671-740)
PARTIALS = ('H', 'H+', 'H-', 'He', 'He+', 'He++', 'C', 'Al', 'Si', 'Si+', 'Ca', 'Ca+', 'Mg', 'Mg+', 'Fe', 'N', 'O')


class EosTables:
    """Partition functions, ionisation energies, abundances and masses for the equation of state (lsx_eos_tables).
    tpf [npf] K ascending; pf [nelem][6][npf] (or a list of [nstage_e][npf] arrays); eion [nelem][6] eV (or a list);
    nstage [nelem]; abund, amass [99], abundances as read (the library normalises them, witt.py:166-176).  nelem >= 28.
    iter_cap: 0 for the reference's iteration caps, > 0 to stop every loop of the equation of state after that many passes."""

    def __init__(self, tpf, pf, eion, nstage, abund, amass, weight_per_H, iter_cap=0):
        self.tpf = f64(tpf).reshape(-1)
        self.nstage = np.ascontiguousarray(nstage, dtype=np.int32).reshape(-1)
        nelem, npf = self.nstage.shape[0], self.tpf.shape[0]
        if isinstance(pf, np.ndarray) and pf.ndim == 3:
            self.pf = f64(pf, (nelem, 6, npf))
            self.eion = f64(eion, (nelem, 6))
        else:
            self.pf, self.eion = np.zeros((nelem, 6, npf)), np.zeros((nelem, 6))
            for e in range(nelem):
                ns = int(self.nstage[e])
                self.pf[e, :ns] = np.asarray(pf[e], dtype=np.float64).reshape(ns, npf)
                self.eion[e, :ns] = np.asarray(eion[e], dtype=np.float64).reshape(ns)
        self.abund, self.amass = f64(abund, (99,)), f64(amass, (99,))
        self.weight_per_H = float(weight_per_H)
        self.iter_cap = int(iter_cap)

    @property
    def nelem(self):
        return int(self.nstage.shape[0])

    def with_iter_cap(self, iter_cap):
        return EosTables(self.tpf, self.pf, self.eion, self.nstage, self.abund, self.amass, self.weight_per_H, iter_cap)

    @classmethod
    def from_kurucz_xdr(cls, path, abund, amass, weight_per_H, nelem=99):
        """Kurucz's partition functions as witt.init_pf_data reads them (witt.py:91-122): big-endian; uint32 npf, npf doubles;
        then 99 times: uint32, uint32 nstage, nstage * npf doubles, nstage doubles in cm^-1 (converted to eV as witt.py:116-122
        does).  Elements with more than six stages keep their first six (the equation of state reads three at most)."""
        with open(path, 'rb') as f:
            raw = f.read()
        pos = 0

        def take(dtype, count):
            nonlocal pos
            a = np.frombuffer(raw, dtype=dtype, count=count, offset=pos)
            pos += a.nbytes
            return a
        npf = int(take('>u4', 1)[0])
        tpf = take('>f8', npf).astype(np.float64)
        nstage, pfs, eions = [], [], []
        for _ in range(99):
            take('>u4', 1)
            ns = int(take('>u4', 1)[0])
            pf = take('>f8', ns * npf).astype(np.float64).reshape(ns, npf)
            eion = take('>f8', ns).astype(np.float64) * _HH * _CC
            eion /= _EV
            keep = min(ns, 6)
            nstage.append(keep)
            pfs.append(pf[:keep])
            eions.append(eion[:keep])
        nelem = int(nelem)
        return cls(tpf, pfs[:nelem], eions[:nelem], nstage[:nelem], abund, amass, weight_per_H)

    def to_c(self):
        """-> (LsxEosTables, keepalive)"""
        t = _capi.LsxEosTables()
        t.npf, t.nelem = self.tpf.shape[0], self.nelem
        t.tpf, t.pf, t.eion, t.abund, t.amass = _ptr(self.tpf), _ptr(self.pf), _ptr(self.eion), _ptr(self.abund), _ptr(self.amass)
        t.nstage = self.nstage.ctypes.data_as(C.POINTER(C.c_int32))
        t.weight_per_H, t.iter_cap, t.reserved = self.weight_per_H, self.iter_cap, 0
        return t, self


class EosResult:
    """pgas, pe [ncol][Nspace] in dyn cm^-2, partials [ncol][17][Nspace] in the order PARTIALS (cm^-3, divided by the partition
    function), status [ncol][Nspace]: witt.pe_pg evaluations per point, negative where a loop ended at its cap."""

    def __init__(self, pgas, pe, partials, status):
        self.pgas, self.pe, self.partials, self.status = pgas, pe, partials, status


def _carrier_problem(Nspace):
    """the smallest problem a context can be made of: the background entries only take Nspace, the device and the stream from it"""
    from .problem import Problem, Transition
    w = np.array([100.0, 200.0, 300.0])
    tr = Transition(0, False, 0, 1, 0, 3, lambda0=300.0, alpha=np.array([1e-23, 2e-23, 3e-23]))
    return Problem(Nspace=int(Nspace), wavelength=w, muz=np.array([1.0]), wmu=np.array([1.0]), Nlevel=[2], trans=[tr],
                   active=np.ones((1, 3), dtype=np.uint8), atom_names=['X'])


class Background:
    """Drop-in for the reference's Background(atmos, spect): .chi, .eta [Nspect][Nspace] and .sca [Nspect][Nspace] (the Thomson
    value on every row, background.py:45-47), computed by the HIP library for spect.wavelength.  `atmos` carries temperature,
    nHTot and ne in SI (it is nondimensionalised for the call and restored, as background.py:23, 53 does, where it has the methods)."""

    def __init__(self, atmos, spect, tables, device=0):
        from .problem import Engine
        self.atmos, self.spect, self.tables = atmos, spect, tables
        nd, dm = getattr(atmos, 'nondimensionalise', None), getattr(atmos, 'dimensionalise', None)
        if nd is not None:
            nd()
        try:
            T, nH, ne = (np.asarray(getattr(atmos, k), dtype=np.float64) for k in ('temperature', 'nHTot', 'ne'))
            eng = Engine(_carrier_problem(T.shape[0]), 1, device=device)
            try:
                chi, eta, sca = eng.background(tables, T, nH, ne, wavelength=np.asarray(spect.wavelength, dtype=np.float64))
            finally:
                eng.close()
        finally:
            if nd is not None and dm is not None:
                dm()
        self.chi, self.eta = chi[0], eta[0]
        self.sca = np.tile(sca[0], (self.chi.shape[0], 1))
