"""Zeeman patterns of spectral lines in LS coupling, for the polarised final pass (include/lsx_hip_stokes.h).

Conventions (those of the reference's model atoms, so that its patterns can be held against these):
  alpha    = M_l - M_u in {-1, 0, +1}: -1 sigma_b (blue), 0 pi, +1 sigma_r (red)
  shift    = g_l M_l - g_u M_u, in units of the normal Zeeman splitting (e / 4 pi m_e) lambda0^2 B / c
  strength   the relative strength of the component, normalised to sum 1 per alpha
Components are listed with M_l outermost and M_u inside it, both ascending.

The Lande factor is g = 3/2 + [S (S + 1) - L (L + 1)] / [2 J (J + 1)] (0 for J = 0).  The unnormalised strengths are the squared
3j symbols of the dipole transition (J_u M_u) -> (J_l M_l) up to a factor common to each alpha (del Toro Iniesta 2003, Table 8.1;
Landi Degl'Innocenti & Landolfi 2004, Table 3.1), written with M = M_u:
  J_u = J_l  (J = J_u):    pi  2 M^2;                    sigma_b (J + M)(J - M + 1);          sigma_r (J - M)(J + M + 1)
  J_u = J_l + 1:           pi  2 [J_u^2 - M^2];          sigma_b (J_u + M)(J_u + M - 1);      sigma_r (J_u - M)(J_u - M - 1)
  J_u = J_l - 1:           pi  2 [(J_u + 1)^2 - M^2];    sigma_b (J_u - M + 1)(J_u - M + 2);  sigma_r (J_u + M + 1)(J_u + M + 2)
`line` is duck-typed: .gLandeEff (or None) and .iLevel / .jLevel (lower / upper) with .J, .L, .S and .lsCoupling."""
from fractions import Fraction

import numpy as np

MAX_COMPONENTS = 64      # LSX_STOKES_MAX_COMPONENTS


class ZeemanComponents:
    """alpha int32 [n], strength float64 [n], shift float64 [n]"""
    __slots__ = ('alpha', 'strength', 'shift')

    def __init__(self, alpha, strength, shift):
        self.alpha = np.ascontiguousarray(alpha, dtype=np.int32)
        self.strength = np.ascontiguousarray(strength, dtype=np.float64)
        self.shift = np.ascontiguousarray(shift, dtype=np.float64)

    def __len__(self):
        return int(self.alpha.shape[0])


def _frac(x):
    return x if isinstance(x, Fraction) else Fraction(x).limit_denominator(2)


def _quantum_numbers(level):
    """-> (J, L, S) as (Fraction, int, Fraction), or None where the level does not carry them (or is not LS coupled)"""
    J, L, S = (getattr(level, k, None) for k in ('J', 'L', 'S'))
    if J is None or L is None or S is None or not getattr(level, 'lsCoupling', True):
        return None
    return _frac(J), int(L), _frac(S)


def lande_factor(J, L, S):
    J, S = _frac(J), _frac(S)
    if J == 0:
        return 0.0
    return 1.5 + float((S * (S + 1) - L * (L + 1)) / (2 * J * (J + 1)))


def _strength(Ju, Mu, Jl, q):
    """unnormalised strength of (J_u M_u) -> (J_l, M_l = M_u + q)"""
    d = Ju - Jl
    if d == 0:
        return (2 * Mu * Mu, (Ju + Mu) * (Ju - Mu + 1), (Ju - Mu) * (Ju + Mu + 1))[(0, -1, 1).index(q)]
    if d == 1:
        return (2 * (Ju * Ju - Mu * Mu), (Ju + Mu) * (Ju + Mu - 1), (Ju - Mu) * (Ju - Mu - 1))[(0, -1, 1).index(q)]
    if d == -1:
        return (2 * ((Ju + 1) ** 2 - Mu * Mu), (Ju - Mu + 1) * (Ju - Mu + 2), (Ju + Mu + 1) * (Ju + Mu + 2))[(0, -1, 1).index(q)]
    raise ValueError('J_u - J_l = %s is no dipole transition' % d)


def _m_values(J):
    return [-J + k for k in range(int(2 * J) + 1)]


def zeeman_components(line):
    """-> ZeemanComponents, or None for a line that has neither gLandeEff nor LS-coupled levels with J, L, S: it stays unpolarised"""
    g_eff = getattr(line, 'gLandeEff', None)
    if g_eff is not None:
        alpha = np.array([-1, 0, 1], dtype=np.int32)
        return ZeemanComponents(alpha, np.ones(3), alpha * float(g_eff))
    lo = _quantum_numbers(getattr(line, 'iLevel', None))
    up = _quantum_numbers(getattr(line, 'jLevel', None))
    if lo is None or up is None:
        return None
    (Jl, Ll, Sl), (Ju, Lu, Su) = lo, up
    gl, gu = lande_factor(Jl, Ll, Sl), lande_factor(Ju, Lu, Su)
    alpha, strength, shift = [], [], []
    norm = {-1: Fraction(0), 0: Fraction(0), 1: Fraction(0)}
    for Ml in _m_values(Jl):
        for Mu in _m_values(Ju):
            q = Ml - Mu
            if abs(q) > 1:
                continue
            s = Fraction(_strength(Ju, Mu, Jl, int(q)))
            alpha.append(int(q))
            strength.append(s)
            shift.append(gl * float(Ml) - gu * float(Mu))
            norm[int(q)] += s
    if not alpha or any(n == 0 for n in norm.values()):
        return None
    strength = [float(s) / float(norm[q]) for s, q in zip(strength, alpha)]
    return ZeemanComponents(alpha, strength, shift)


def effective_lande(line):
    """the effective Lande factor of the line: gLandeEff where it is set, else (g_u + g_l) / 2 + (g_u - g_l) [J_u (J_u + 1) -
    J_l (J_l + 1)] / 4; None where the levels lack the quantum numbers"""
    g_eff = getattr(line, 'gLandeEff', None)
    if g_eff is not None:
        return g_eff
    lo = _quantum_numbers(getattr(line, 'iLevel', None))
    up = _quantum_numbers(getattr(line, 'jLevel', None))
    if lo is None or up is None:
        return None
    (Jl, Ll, Sl), (Ju, Lu, Su) = lo, up
    gl, gu = lande_factor(Jl, Ll, Sl), lande_factor(Ju, Lu, Su)
    return 0.5 * (gu + gl) + 0.25 * (gu - gl) * float(Ju * (Ju + 1) - Jl * (Jl + 1))


def pack(patterns, nlines):
    """patterns: None, or one entry per line (None / a ZeemanComponents / an (alpha, strength, shift) triple) -> the arrays
    lsx_hip_stokes_rays takes: (ncomp int32 [nlines], alpha int32 [sum], strength [sum], shift [sum]); the three have at least one
    element"""
    if patterns is None:
        patterns = [None] * nlines
    patterns = list(patterns)
    if len(patterns) != nlines:
        raise ValueError('%d patterns for %d lines' % (len(patterns), nlines))
    ncomp = np.zeros(max(nlines, 1), dtype=np.int32)
    al, st, sh = [np.zeros(0, dtype=np.int32)], [np.zeros(0)], [np.zeros(0)]
    for l, p in enumerate(patterns):
        if p is None:
            continue
        if not isinstance(p, ZeemanComponents):
            p = ZeemanComponents(*p)
        if not (p.alpha.shape == p.strength.shape == p.shift.shape and p.alpha.ndim == 1):
            raise ValueError('pattern of line %d: alpha, strength and shift differ in shape' % l)
        ncomp[l] = len(p)
        al.append(p.alpha); st.append(p.strength); sh.append(p.shift)
    cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts + [np.zeros(1, dtype=dt)]), dtype=dt)
    return ncomp, cat(al, np.int32), cat(st, np.float64), cat(sh, np.float64)
