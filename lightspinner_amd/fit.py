"""Fitting the magnetic field vector to observed Stokes profiles (include/lsx_hip_fit.h): what the callers of Engine.fit_field_normal,
Engine.fit_field_chi2, Engine.fit_field_step and drivers.fit_field_columns share -- the parameterisation's helpers and the result
classes.  The sums and the solve are the library's; nothing here computes.  `Instrument` is the banded matrix of
include/lsx_hip_fit.h (lsx_fit_instrument) with its constructors: set-up that runs once, on the host, like hat_basis."""
import math

import numpy as np

PARAMETERS = ('B', 'gammaB', 'chiB')
VELOCITY_PARAMETERS = PARAMETERS + ('vlos',)          # with the line-of-sight velocity as the fourth quantity (nnode of four counts)
MAX_PARAMS = 24                       # LSX_FIT_MAX_PARAMS
# status of a column of FieldFit
CONVERGED, LAMBDA_CEILING, MAX_ITER = 0, 1, 2


def hat_basis(coordinate, node_positions):
    """The piecewise-linear partition of unity over `coordinate` [Nspace] (a depth index, a height, log tau: anything monotonic) with
    nodes at `node_positions` (strictly increasing, in the coordinate's units): -> [n][Nspace], row i is 1 at node i and falls
    linearly to 0 at its neighbours; outside the nodes the first and the last row stay 1.  One node: a constant.  The rows sum to 1
    at every depth, so node values ARE field values at the nodes."""
    x = np.asarray(coordinate, dtype=np.float64).reshape(-1)
    t = np.asarray(node_positions, dtype=np.float64).reshape(-1)
    if t.shape[0] < 1 or np.any(np.diff(t) <= 0) or not (np.all(np.isfinite(t)) and np.all(np.isfinite(x))):
        raise ValueError('hat_basis: the node positions must be finite and strictly increasing, the coordinate finite')
    out = np.zeros((t.shape[0], x.shape[0]), dtype=np.float64)
    if t.shape[0] == 1:
        out[0] = 1.0
        return out
    xc = np.clip(x, t[0], t[-1])
    seg = np.clip(np.searchsorted(t, xc, side='right') - 1, 0, t.shape[0] - 2)
    f = (xc - t[seg]) / (t[seg + 1] - t[seg])
    k = np.arange(x.shape[0])
    out[seg, k] = 1.0 - f
    out[seg + 1, k] += f
    return out


def stack_basis(B=None, gammaB=None, chiB=None, vlos=None):
    """-> (basis [P][Nspace], nnode (3 ints)) from the parameters' own row sets (None: not fitted), in the library's order; with
    `vlos` rows (the line-of-sight velocity is fitted too: include/lsx_hip_stokes_velocity.h) nnode has 4 ints"""
    rows = [None if b is None else np.atleast_2d(np.asarray(b, dtype=np.float64)) for b in (B, gammaB, chiB)]
    if vlos is not None:
        rows.append(np.atleast_2d(np.asarray(vlos, dtype=np.float64)))
    if all(r is None for r in rows):
        raise ValueError('stack_basis: no parameter is fitted')
    return np.concatenate([r for r in rows if r is not None], axis=0), tuple(0 if r is None else r.shape[0] for r in rows)


class Instrument:
    """The instrument of the field fit (include/lsx_hip_fit.h, lsx_fit_instrument): pixel o reads the `width` wavelengths of the window
    from first[o] on, S'[o] = sum_i weight[o][i] S[first[o] + i].  first [nobs] ints with 0 <= first[o] <= nla - width, weight
    [nobs][width] finite (a shorter row padded with zeros), nla the wavelengths of the window.  .nobs, .width, .matrix()."""

    def __init__(self, first, weight, nla):
        self.first = np.ascontiguousarray(np.asarray(first).reshape(-1), dtype=np.int32)
        self.weight = np.ascontiguousarray(np.atleast_2d(np.asarray(weight, dtype=np.float64)))
        self.nla = int(nla)
        if self.weight.ndim != 2 or self.weight.shape[0] != self.first.shape[0] or self.first.shape[0] < 1:
            raise ValueError('Instrument: weight must be [nobs][width] with one row per entry of first, nobs >= 1')
        if not 1 <= self.weight.shape[1] <= self.nla:
            raise ValueError('Instrument: width = %d is outside [1, nla = %d]' % (self.weight.shape[1], self.nla))
        if np.any(self.first < 0) or np.any(self.first > self.nla - self.weight.shape[1]):
            raise ValueError('Instrument: a pixel reads outside the window: first must lie in [0, nla - width]')
        if not np.all(np.isfinite(self.weight)):
            raise ValueError('Instrument: the weights must be finite')

    nobs = property(lambda self: self.weight.shape[0])
    width = property(lambda self: self.weight.shape[1])

    def matrix(self):
        """the dense [nobs][nla] array (tests, plots)"""
        K = np.zeros((self.nobs, self.nla))
        for o in range(self.nobs):
            K[o, self.first[o]:self.first[o] + self.width] = self.weight[o]
        return K

    @classmethod
    def identity(cls, nla):
        return cls(np.arange(int(nla)), np.ones((int(nla), 1)), nla)

    @classmethod
    def from_matrix(cls, K):
        """any dense [nobs][nla] array: a pixel's band is the span of its non-zeros, width the largest span; the starts are shifted
        so that every band fits inside the window.  .matrix() gives K back exactly."""
        K = np.atleast_2d(np.asarray(K, dtype=np.float64))
        if K.ndim != 2 or K.shape[0] < 1 or K.shape[1] < 1 or not np.all(np.isfinite(K)):
            raise ValueError('Instrument.from_matrix: a finite [nobs][nla] array is needed')
        nobs, nla = K.shape
        lo, hi = np.zeros(nobs, dtype=np.int64), np.zeros(nobs, dtype=np.int64)            # [lo, hi]: the span (an empty row: 0, 0)
        for o in range(nobs):
            nz = np.nonzero(K[o])[0]
            if nz.shape[0]:
                lo[o], hi[o] = nz[0], nz[-1]
        width = int(np.max(hi - lo)) + 1
        first = np.minimum(lo, nla - width)
        return cls(first, np.stack([K[o, first[o]:first[o] + width] for o in range(nobs)]), nla)

    @staticmethod
    def _grid(who, grid, pixels):
        x = np.asarray(grid, dtype=np.float64).reshape(-1)
        t = np.asarray(pixels, dtype=np.float64).reshape(-1)
        if x.shape[0] < 1 or t.shape[0] < 1 or not (np.all(np.isfinite(x)) and np.all(np.isfinite(t))):
            raise ValueError('%s: grid and pixels must be finite and not empty' % who)
        if np.any(np.diff(x) <= 0):
            raise ValueError('%s: the grid must be strictly increasing' % who)
        if np.any(t < x[0]) or np.any(t > x[-1]):
            raise ValueError('%s: a pixel lies outside the grid [%r, %r]' % (who, x[0], x[-1]))
        return x, t

    @classmethod
    def sampling(cls, grid, pixels):
        """linear interpolation of the window's wavelengths `grid` [nla] at `pixels` [nobs]: two weights a pixel, exactly what
        np.interp applies"""
        x, t = cls._grid('Instrument.sampling', grid, pixels)
        eye = np.eye(x.shape[0])
        return cls.from_matrix(np.stack([np.interp(t, x, eye[i]) for i in range(x.shape[0])], axis=1))

    @classmethod
    def gaussian(cls, grid, pixels, fwhm, nsigma=4.0):
        """A Gaussian line-spread function of full width `fwhm` (the grid's units) centred on each pixel, cut at nsigma standard
        deviations and at the grid's ends, folded with the piecewise-linear interpolant of the spectrum between the grid points:
        raw[o][i] = integral of hat_i(l) g(l_o - l) dl in closed form (erf and exp per interval), each row divided by its sum, so that
        a flat continuum stays flat.  The grid must resolve the line as well as the pixels do: the interpolant is linear."""
        x, t = cls._grid('Instrument.gaussian', grid, pixels)
        if not (np.isfinite(fwhm) and fwhm > 0 and np.isfinite(nsigma) and nsigma > 0):
            raise ValueError('Instrument.gaussian: fwhm and nsigma must be finite and positive (Instrument.sampling has no smearing)')
        sigma = float(fwhm) / (2.0 * math.sqrt(2.0 * math.log(2.0)))
        K = np.zeros((t.shape[0], x.shape[0]))
        if x.shape[0] == 1:
            K[:, 0] = 1.0
            return cls.from_matrix(K)
        r2, rpi = math.sqrt(2.0), math.sqrt(2.0 * math.pi)
        for o, c in enumerate(t):
            a, b = max(x[0], c - nsigma * sigma), min(x[-1], c + nsigma * sigma)
            j0 = max(int(np.searchsorted(x, a, side='right')) - 1, 0)
            for j in range(j0, x.shape[0] - 1):
                lo, hi = max(x[j], a), min(x[j + 1], b)
                if lo >= b:
                    break
                if hi <= lo:
                    continue
                tl, tr = (lo - c) / sigma, (hi - c) / sigma
                # G0 = integral of g, E1 = integral of (l - l_o) g over [lo, hi]; the difference of two erfc on one side of the centre
                # (no cancellation in the wings), of two erf across it
                if tl >= 0:
                    G0 = 0.5 * (math.erfc(tl / r2) - math.erfc(tr / r2))
                elif tr <= 0:
                    G0 = 0.5 * (math.erfc(-tr / r2) - math.erfc(-tl / r2))
                else:
                    G0 = 0.5 * (math.erf(tr / r2) - math.erf(tl / r2))
                E1 = sigma / rpi * (math.exp(-0.5 * tl * tl) - math.exp(-0.5 * tr * tr))
                h = x[j + 1] - x[j]
                K[o, j] += ((x[j + 1] - c) * G0 - E1) / h
                K[o, j + 1] += (E1 + (c - x[j]) * G0) / h
            tot = K[o].sum()
            if not tot > 0:
                raise ValueError('Instrument.gaussian: pixel %d gathers nothing from the grid' % o)
            K[o] /= tot
        return cls.from_matrix(K)


class FieldNormal:
    """What fit_field_normal returns: .chi2 [ncol], .grad [ncol][P], .hess [ncol][P][P], .field [ncol][3][Nspace] (the expanded
    field: B, gammaB, chiB; with nnode of four counts [ncol][4][Nspace], the fourth row vlos)."""

    def __init__(self, chi2, grad, hess, field):
        self.chi2, self.grad, self.hess, self.field = chi2, grad, hess, field


class FieldFit:
    """What drivers.fit_field_columns returns: .nodes [ncol][P], .field [ncol][3][Nspace] (expanded from them; [4] with vlos), .chi2 [ncol],
    .history [iterations + 1][ncol] (chi2 at the nodes held after each iteration; row 0 the start), .lam [ncol],
    .iterations [ncol] (those a column took part in), .status [ncol]: fit.CONVERGED, fit.LAMBDA_CEILING or fit.MAX_ITER, and
    .nnode.  Context.fit_field drops the column axis."""

    def __init__(self, nodes, field, chi2, history, lam, iterations, status, nnode):
        self.nodes, self.field, self.chi2, self.history = nodes, field, chi2, history
        self.lam, self.iterations, self.status, self.nnode = lam, iterations, status, tuple(int(n) for n in nnode)

    def parameter(self, name):
        """the nodes of 'B', 'gammaB', 'chiB' or (fitted with four quantities) 'vlos': [ncol][nnode]"""
        i = VELOCITY_PARAMETERS[:len(self.nnode)].index(name)
        o = sum(self.nnode[:i])
        return self.nodes[..., o:o + self.nnode[i]]
