"""Radiation boundary conditions of a column (include/lsx_hip_boundary.h): what a ray starts with at each end.

Kinds: 'zero', 'thermalised', 'given'.  They are accepted as strings (any case, also 'thermalized'), as the LSX_BOUNDARY_*
integers, or as any object with a `.name` -- the reference's BoundaryCondition.Zero / .Thermalised members match by name, without
the reference being imported."""
import numpy as np

ZERO, THERMALISED, GIVEN = 0, 1, 2
KIND_NAMES = ('zero', 'thermalised', 'given')
_ALIASES = {'zero': ZERO, 'thermalised': THERMALISED, 'thermalized': THERMALISED, 'given': GIVEN}


def kind_code(kind):
    """'zero' / 'thermalised' / 'given', an LSX_BOUNDARY_* integer or an enum-like object with .name -> the integer"""
    if isinstance(kind, (bool, np.bool_)):
        raise ValueError('boundary kind %r: expected one of %s' % (kind, ', '.join(KIND_NAMES)))
    if isinstance(kind, (int, np.integer)):
        if int(kind) not in (ZERO, THERMALISED, GIVEN):
            raise ValueError('boundary kind %d: expected 0 (zero), 1 (thermalised) or 2 (given)' % int(kind))
        return int(kind)
    name = kind if isinstance(kind, str) else getattr(kind, 'name', None)
    if not isinstance(name, str) or name.strip().lower() not in _ALIASES:
        raise ValueError('boundary kind %r: expected one of %s' % (kind, ', '.join(KIND_NAMES)))
    return _ALIASES[name.strip().lower()]


def _array(a, kind, which, shape, lead):
    """the array of one end against its kind: required exactly where the kind is 'given'; -> float64 C-contiguous, or None"""
    if kind == GIVEN and a is None:
        raise ValueError('the %s boundary is given: I_%s is needed' % (which, which))
    if kind != GIVEN and a is not None:
        raise ValueError('I_%s was handed over, but the %s boundary is %s' % (which, which, KIND_NAMES[kind]))
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        if lead is not None and a.shape == tuple(shape):           # one column's array for every column of the range
            a = np.ascontiguousarray(np.broadcast_to(a, (lead,) + tuple(shape)))
        want = tuple(shape) if lead is None else (lead,) + tuple(shape)
        if a.shape != want:
            raise ValueError('I_%s has shape %s, expected %s' % (which, a.shape, want))
    elif a.ndim != 2:
        raise ValueError('I_%s has shape %s, expected [Nspect][Nrays]' % (which, a.shape))
    return a


class Boundary:
    """The boundary of ONE column: Boundary(lower, upper, I_lower=None, I_upper=None).  lower: where up-going rays start (the
    deepest point), upper: where down-going rays start.  I_lower / I_upper [Nspect][Nrays], SI units as the intensity the library
    returns, on the context's wavelengths and rays: needed exactly where the kind is 'given'."""

    def __init__(self, lower='thermalised', upper='zero', I_lower=None, I_upper=None):
        self.lower = kind_code(lower)
        self.upper = kind_code(upper)
        self.I_lower = _array(I_lower, self.lower, 'lower', None, None)
        self.I_upper = _array(I_upper, self.upper, 'upper', None, None)
        if self.I_lower is not None and self.I_upper is not None and self.I_lower.shape != self.I_upper.shape:
            raise ValueError('I_lower %s and I_upper %s differ in shape' % (self.I_lower.shape, self.I_upper.shape))

    @classmethod
    def from_atmos(cls, atmos):
        """the kinds an atmosphere carries (the reference's Atmosphere.lowerBc / .upperBc, which its own solver ignores)"""
        return cls(getattr(atmos, 'lowerBc'), getattr(atmos, 'upperBc'))

    @property
    def is_default(self):
        return self.lower == THERMALISED and self.upper == ZERO

    def __repr__(self):
        return 'Boundary(lower=%r, upper=%r)' % (KIND_NAMES[self.lower], KIND_NAMES[self.upper])
