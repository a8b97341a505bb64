"""The depth scales of an atmosphere on the GPU: the reference's AtmosphereConstructor.convert_scales (atmosphere.py:70-144) --
column mass, geometric height and the optical depth at 500 nm from whichever of them the model is tabulated on -- through
include/lsx_hip_scales.h.

    tables = EosTables.from_kurucz_xdr('pf_Kurucz.input', abund, amass, weight_per_H)
    convert_scales(atmos, tables)             # sets atmos.cmass, atmos.height, atmos.tau_ref

For many columns, or to put the heights straight into an engine without a copy through the host, use Engine.convert_scales
(problem.py).  The reference's Atmosphere object, its units and its quadrature are not restated here.
"""
import numpy as np

from . import _capi

_SCALES = {'geometric': _capi.LSX_SCALE_GEOMETRIC, 'column_mass': _capi.LSX_SCALE_COLUMN_MASS, 'tau500': _capi.LSX_SCALE_TAU500,
           # ScaleType's names (atmosphere.py:13-16)
           'Geometric': _capi.LSX_SCALE_GEOMETRIC, 'ColumnMass': _capi.LSX_SCALE_COLUMN_MASS, 'Tau500': _capi.LSX_SCALE_TAU500}


def scale_code(scale):
    """'geometric' / 'column_mass' / 'tau500', a ScaleType-like object (by its .name) or an LSX_SCALE_* value -> LSX_SCALE_*"""
    name = getattr(scale, 'name', scale)
    if isinstance(name, str):
        if name not in _SCALES:
            raise ValueError('unknown depth scale %r' % (name,))
        return _SCALES[name]
    return int(name)            # (the library refuses a value outside its enum)


class Scales:
    """height [m] (zero where tau500 = 1, except on the geometric scale, whose heights are returned as given), cmass [kg m^-2],
    tau_ref (tau500) and chi_ref (the continuous opacity at 500 nm, m^-1), each [ncol][Nspace]"""

    def __init__(self, height, cmass, tau_ref, chi_ref):
        self.height, self.cmass, self.tau_ref, self.chi_ref = height, cmass, tau_ref, chi_ref


def convert_scales(atmos, tables, logG=2.44, device=0):
    """Drop-in for AtmosphereConstructor.convert_scales on a Lightspinner-shaped constructor: reads .depthScale, .scale (by its
    .name: Geometric, ColumnMass, Tau500), .temperature, .nHTot and .ne, sets .cmass, .height and .tau_ref (SI, [Nspace]) and
    returns the object.  It is nondimensionalised for the call and restored where it has the methods (atmosphere.py:71, 143)."""
    from .background import _carrier_problem
    from .problem import Engine
    nd, dm = getattr(atmos, 'nondimensionalise', None), getattr(atmos, 'dimensionalise', None)
    if nd is not None:
        nd()
    try:
        ds = np.asarray(atmos.depthScale, dtype=np.float64)
        ne = getattr(atmos, 'ne', None)
        eng = Engine(_carrier_problem(ds.shape[0]), 1, device=device)
        try:
            r = eng.convert_scales(tables, atmos.scale, ds, np.asarray(atmos.temperature, dtype=np.float64),
                                   np.asarray(atmos.nHTot, dtype=np.float64), None if ne is None else np.asarray(ne, dtype=np.float64),
                                   logG=logG)
        finally:
            eng.close()
        atmos.cmass, atmos.height, atmos.tau_ref = r.cmass[0], r.height[0], r.tau_ref[0]
    finally:
        if nd is not None and dm is not None:
            dm()
    return atmos
