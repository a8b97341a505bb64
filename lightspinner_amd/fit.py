"""Fitting the magnetic field vector to observed Stokes profiles (include/lsx_hip_fit.h): what the callers of Engine.fit_field_normal,
Engine.fit_field_chi2, Engine.fit_field_step and drivers.fit_field_columns share -- the parameterisation's helpers and the result
classes.  The sums and the solve are the library's; nothing here computes.  `Instrument` is the banded matrix of
include/lsx_hip_fit.h (lsx_fit_instrument) with its constructors: set-up that runs once, on the host, like hat_basis.  `Penalty` is the
constant matrix of include/lsx_hip_fit_regular.h (lsx_fit_penalty) with its constructors, `FieldUncertainty` what
Engine.fit_field_uncertainty returns."""
import math

import numpy as np

PARAMETERS = ('B', 'gammaB', 'chiB')
VELOCITY_PARAMETERS = PARAMETERS + ('vlos',)          # with the line-of-sight velocity as the fourth quantity (nnode of four counts)
MAX_PARAMS = 24                       # LSX_FIT_MAX_PARAMS
MAX_PENALTY_ROWS = 96                 # LSX_REGULAR_MAX_ROWS
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


def _per_parameter(who, what, given, nnode, default):
    """a dict from parameter names, or a sequence in the library's order -> one entry per count of nnode (`default` where missing)"""
    names = VELOCITY_PARAMETERS[:len(nnode)]
    if isinstance(given, dict):
        unknown = [k for k in given if k not in names]
        if unknown:
            raise ValueError('%s: %s names %r; the parameters are %r' % (who, what, unknown, names))
        return [given.get(n, default) for n in names]
    # a sequence is told from a scalar without making one array of it: the parameters' entries may differ in length
    if isinstance(given, np.ndarray):
        given = list(given) if given.ndim else [given[()]]
    else:
        given = list(given) if isinstance(given, (list, tuple)) else [given]
    if len(given) > len(names):
        raise ValueError('%s: %s has %d entries for %d parameters' % (who, what, len(given), len(names)))
    return given + [default] * (len(names) - len(given))


def _counts(who, nnode):
    nn = tuple(int(n) for n in nnode)
    if len(nn) not in (3, 4) or min(nn) < 0 or not 1 <= sum(nn) <= MAX_PARAMS:
        raise ValueError('%s: nnode must hold three or four counts >= 0 that sum to 1 .. %d, not %r' % (who, MAX_PARAMS, nn))
    return nn


def _alphas(who, alpha, nn):
    al = [0.0 if a is None else float(a) for a in _per_parameter(who, 'alpha', alpha, nn, 0.0)]
    if not all(np.isfinite(a) and a >= 0 for a in al):
        raise ValueError('%s: every alpha must be finite and not negative' % who)
    return al


class Penalty:
    """The quadratic penalty of a regularised field fit (include/lsx_hip_fit_regular.h, lsx_fit_penalty): Q extra data points of unit
    weight whose Jacobian is the constant matrix L.  The pseudo-residual of row q of a column is target[q] - sum_j L[q][j] nodes[j],
    the penalty the sum of their squares: it is added to chi2.  L [Q][P] finite, 1 <= Q <= 96, the columns in the order of the nodes
    (B's first); target [Q] (all columns alike), [ncol][Q], or None for zeros.  .nrow, .nparam.
    A row that measures some combination of the nodes with the standard deviation sigma -- in the units of the fit's weights, i.e.
    when the weights are 1 / noise^2 -- is that combination's coefficients times 1 / sigma: in the constructors below `alpha` is
    1 / sigma^2 of what the row measures."""

    def __init__(self, L, target=None):
        self.L = np.ascontiguousarray(np.atleast_2d(np.asarray(L, dtype=np.float64)))
        if self.L.ndim != 2 or not 1 <= self.L.shape[0] <= MAX_PENALTY_ROWS or not 1 <= self.L.shape[1] <= MAX_PARAMS:
            raise ValueError('Penalty: L must be [Q][P] with 1 <= Q <= %d and 1 <= P <= %d, not %r'
                             % (MAX_PENALTY_ROWS, MAX_PARAMS, self.L.shape))
        if not np.all(np.isfinite(self.L)):
            raise ValueError('Penalty: L must be finite')
        self.target = None
        if target is not None:
            self.target = np.ascontiguousarray(np.asarray(target, dtype=np.float64))
            if self.target.ndim not in (1, 2) or self.target.shape[-1] != self.L.shape[0]:
                raise ValueError('Penalty: target must be [Q] or [ncol][Q] with Q = %d, not %r' % (self.L.shape[0], self.target.shape))
            if not np.all(np.isfinite(self.target)):
                raise ValueError('Penalty: target must be finite')

    nrow = property(lambda self: self.L.shape[0])
    nparam = property(lambda self: self.L.shape[1])

    def targets(self, ncol):
        """target as [ncol][Q], or None"""
        if self.target is None:
            return None
        if self.target.ndim == 2 and self.target.shape[0] not in (1, ncol):
            raise ValueError('Penalty: target is made for %d columns, the call has %d' % (self.target.shape[0], ncol))
        return np.ascontiguousarray(np.broadcast_to(self.target, (ncol, self.nrow)))

    @classmethod
    def smoothness(cls, nnode, alpha, order=2, positions=None):
        """Per parameter p with alpha_p > 0 and at least order + 1 nodes, one row per run of order + 1 neighbouring nodes, times
        sqrt(alpha_p); target zero.  order 1: the divided difference (x[i+1] - x[i]) / (t[i+1] - t[i]); order 2: the second derivative
        by divided differences, ((x[i+2] - x[i+1]) / h1 - (x[i+1] - x[i]) / h0) / ((h0 + h1) / 2) -- x[i] - 2 x[i+1] + x[i+2] at unit
        spacing.  positions: the nodes' coordinates t per parameter (a dict from names or a sequence in the library's order; strictly
        increasing), None: unit spacing.  With positions a field that is linear in the coordinate has zero second-order penalty.
        alpha: a dict from parameter names ('B', 'gammaB', 'chiB', 'vlos') or a sequence in that order; a missing or zero entry gives
        no rows.  alpha_p is 1 / sigma^2 of the difference the row measures, in the units of the fit's weights: with weights
        1 / noise^2, alpha_B = 1e6 T^-2 says that second differences of the B nodes are expected to be about 1e-3 T."""
        who = 'Penalty.smoothness'
        nn = _counts(who, nnode)
        if order not in (1, 2):
            raise ValueError('%s: order must be 1 or 2' % who)
        al = _alphas(who, alpha, nn)
        pos = [None] * len(nn) if positions is None else _per_parameter(who, 'positions', positions, nn, None)
        LD = np.longdouble
        rows, P, o = [], sum(nn), 0
        for n, a, t in zip(nn, al, pos):
            if a > 0 and n >= order + 1:
                t = np.arange(n, dtype=LD) if t is None else np.asarray(t, dtype=np.float64).reshape(-1).astype(LD)
                if t.shape[0] != n or not np.all(np.isfinite(t)) or np.any(np.diff(t) <= 0):
                    raise ValueError('%s: a parameter with %d nodes needs %d finite, strictly increasing positions' % (who, n, n))
                w = np.sqrt(LD(a))
                for i in range(n - order):
                    r = np.zeros(P)
                    if order == 1:
                        r[o + i + 1] = float(w / (t[i + 1] - t[i]))          # one rounding; the pair is exactly opposite
                        r[o + i] = -r[o + i + 1]
                    else:
                        h0, h1 = t[i + 1] - t[i], t[i + 2] - t[i + 1]
                        r[o + i] = float(2 * w / (h0 * (h0 + h1)))           # formed in extended precision, rounded once
                        r[o + i + 1] = float(-2 * w / (h0 * h1))
                        r[o + i + 2] = float(2 * w / (h1 * (h0 + h1)))
                    rows.append(r)
            o += n
        if not rows:
            raise ValueError('%s: no rows: every alpha is zero or no parameter has %d nodes' % (who, order + 1))
        return cls(np.stack(rows))

    @classmethod
    def prior(cls, nnode, alpha, values):
        """Per parameter p with alpha_p > 0, one row per node: sqrt(alpha_p) e_j with the target sqrt(alpha_p) value_j -- the node
        is expected at `value` within sigma = 1 / sqrt(alpha_p), in the units of the fit's weights.  values: the nodes' expected
        values, [P] or [ncol][P] in the nodes' order, or a dict from parameter names to [n_p] or [ncol][n_p].  alpha as in smoothness."""
        who = 'Penalty.prior'
        nn = _counts(who, nnode)
        al = _alphas(who, alpha, nn)
        P, off = sum(nn), np.cumsum([0] + list(nn))
        names = VELOCITY_PARAMETERS[:len(nn)]
        if isinstance(values, dict):
            parts = {k: np.asarray(v, dtype=np.float64) for k, v in values.items()}
            lead = max([v.shape[:-1] for v in parts.values() if v.ndim > 1] or [()], key=len)
            full = np.zeros(lead + (P,))
            for i, name in enumerate(names):
                if al[i] > 0 and nn[i] > 0:
                    if name not in parts:
                        raise ValueError('%s: alpha names %r, values does not' % (who, name))
                    full[..., off[i]:off[i + 1]] = parts[name]
            values = full
        values = np.asarray(values, dtype=np.float64)
        if values.ndim not in (1, 2) or values.shape[-1] != P:
            raise ValueError('%s: values must be [P] or [ncol][P] with P = %d, not %r' % (who, P, values.shape))
        rows, cols = [], []
        for i in range(len(nn)):
            for j in range(off[i], off[i + 1]):
                if al[i] > 0:
                    r = np.zeros(P)
                    r[j] = np.sqrt(al[i])
                    rows.append(r)
                    cols.append(j)
        if not rows:
            raise ValueError('%s: no rows: every alpha is zero' % who)
        L = np.stack(rows)
        return cls(L, values[..., cols] * L[np.arange(len(cols)), cols])

    @classmethod
    def stack(cls, *penalties):
        """the rows of several penalties of one parameterisation, one below the other"""
        if not penalties or len({p.nparam for p in penalties}) != 1:
            raise ValueError('Penalty.stack: at least one penalty, all with the same number of nodes')
        L = np.concatenate([p.L for p in penalties], axis=0)
        if all(p.target is None for p in penalties):
            return cls(L)
        ncols = {p.target.shape[0] for p in penalties if p.target is not None and p.target.ndim == 2}
        if len(ncols) > 1:
            raise ValueError('Penalty.stack: the targets are made for different column counts %r' % sorted(ncols))
        lead = (ncols.pop(),) if ncols else ()
        return cls(L, np.concatenate([np.zeros(lead + (p.nrow,)) if p.target is None else np.broadcast_to(p.target, lead + (p.nrow,))
                                      for p in penalties], axis=-1))


class FieldUncertainty:
    """What Engine.fit_field_uncertainty returns (include/lsx_hip_fit_regular.h, lsx_hip_regular_uncertainty): .ainv [ncol][P][P] (the
    inverse of hess + L^T L, column by column), .cov [ncol][P][P] (the sandwich ainv hess ainv, times the scale; without a penalty
    ainv itself), .sigma [ncol][P] = sqrt(diag cov), .field_sigma [ncol][npar][Nspace] (the standard deviation of the expanded field at
    every depth, 0 for a parameter without nodes), .status [ncol] (1: the system is singular or holds a NaN; that column is NaN) and
    .nnode.  Context.fit_field drops the column axis."""

    def __init__(self, ainv, cov, sigma, field_sigma, status, nnode):
        self.ainv, self.cov, self.sigma, self.field_sigma, self.status = ainv, cov, sigma, field_sigma, status
        self.nnode = tuple(int(n) for n in nnode)

    def parameter(self, name):
        """sigma of the nodes of 'B', 'gammaB', 'chiB' or 'vlos': [ncol][nnode]"""
        i = VELOCITY_PARAMETERS[:len(self.nnode)].index(name)
        o = sum(self.nnode[:i])
        return self.sigma[..., o:o + self.nnode[i]]

    def correlation(self):
        """cov[a][b] / (sigma[a] sigma[b]): [ncol][P][P], for reading"""
        with np.errstate(divide='ignore', invalid='ignore'):
            return self.cov / (self.sigma[..., :, None] * self.sigma[..., None, :])


class FieldNormal:
    """What fit_field_normal returns: .chi2 [ncol], .grad [ncol][P], .hess [ncol][P][P], .field [ncol][3][Nspace] (the expanded
    field: B, gammaB, chiB; with nnode of four counts [ncol][4][Nspace], the fourth row vlos)."""

    def __init__(self, chi2, grad, hess, field):
        self.chi2, self.grad, self.hess, self.field = chi2, grad, hess, field


class FieldFit:
    """What drivers.fit_field_columns returns: .nodes [ncol][P], .field [ncol][3][Nspace] (expanded from them; [4] with vlos), .chi2 [ncol],
    .history [iterations + 1][ncol] (chi2 at the nodes held after each iteration; row 0 the start), .lam [ncol],
    .iterations [ncol] (those a column took part in), .status [ncol]: fit.CONVERGED, fit.LAMBDA_CEILING or fit.MAX_ITER, and
    .nnode.  With a penalty .chi2 and .history are the objective the loop minimises, data plus penalty; .penalty [ncol] is the
    penalty's part (zeros without one) and .chi2_data [ncol] the data's.  .dof [ncol]: the points of positive weight minus P, counted
    when first asked for (None if the loop was not told the data's shape); .uncertainty: a FieldUncertainty, None unless asked for.
    Context.fit_field drops the column axis."""

    def __init__(self, nodes, field, chi2, history, lam, iterations, status, nnode, penalty=None, chi2_data=None, uncertainty=None,
                 dof=None):
        self.nodes, self.field, self.chi2, self.history = nodes, field, chi2, history
        self.lam, self.iterations, self.status, self.nnode = lam, iterations, status, tuple(int(n) for n in nnode)
        self.penalty = np.zeros_like(np.asarray(chi2, dtype=np.float64)) if penalty is None else penalty
        self.chi2_data = chi2 if chi2_data is None else chi2_data
        self.uncertainty, self._dof = uncertainty, dof

    @property
    def dof(self):
        """the points of positive weight minus P, counted when first asked for"""
        if callable(self._dof):
            self._dof = self._dof()
        return self._dof

    def parameter(self, name):
        """the nodes of 'B', 'gammaB', 'chiB' or (fitted with four quantities) 'vlos': [ncol][nnode]"""
        i = VELOCITY_PARAMETERS[:len(self.nnode)].index(name)
        o = sum(self.nnode[:i])
        return self.nodes[..., o:o + self.nnode[i]]
