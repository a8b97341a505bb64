"""Fitting the magnetic field vector to observed Stokes profiles (include/lsx_hip_fit.h): what the callers of Engine.fit_field_normal,
Engine.fit_field_chi2, Engine.fit_field_step and drivers.fit_field_columns share -- the parameterisation's helpers and the result
classes.  The sums and the solve are the library's; nothing here computes."""
import numpy as np

PARAMETERS = ('B', 'gammaB', 'chiB')
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


def stack_basis(B=None, gammaB=None, chiB=None):
    """-> (basis [P][Nspace], nnode (3 ints)) from the parameters' own row sets (None: not fitted), in the library's order"""
    rows = [None if b is None else np.atleast_2d(np.asarray(b, dtype=np.float64)) for b in (B, gammaB, chiB)]
    if all(r is None for r in rows):
        raise ValueError('stack_basis: no parameter is fitted')
    return np.concatenate([r for r in rows if r is not None], axis=0), tuple(0 if r is None else r.shape[0] for r in rows)


class FieldNormal:
    """What fit_field_normal returns: .chi2 [ncol], .grad [ncol][P], .hess [ncol][P][P], .field [ncol][3][Nspace] (the expanded
    field: B, gammaB, chiB)."""

    def __init__(self, chi2, grad, hess, field):
        self.chi2, self.grad, self.hess, self.field = chi2, grad, hess, field


class FieldFit:
    """What drivers.fit_field_columns returns: .nodes [ncol][P], .field [ncol][3][Nspace] (expanded from them), .chi2 [ncol],
    .history [iterations + 1][ncol] (chi2 at the nodes held after each iteration; row 0 the start), .lam [ncol],
    .iterations [ncol] (those a column took part in), .status [ncol]: fit.CONVERGED, fit.LAMBDA_CEILING or fit.MAX_ITER, and
    .nnode.  Context.fit_field drops the column axis."""

    def __init__(self, nodes, field, chi2, history, lam, iterations, status, nnode):
        self.nodes, self.field, self.chi2, self.history = nodes, field, chi2, history
        self.lam, self.iterations, self.status, self.nnode = lam, iterations, status, tuple(int(n) for n in nnode)

    def parameter(self, name):
        """the nodes of 'B', 'gammaB' or 'chiB': [ncol][nnode]"""
        i = PARAMETERS.index(name)
        o = sum(self.nnode[:i])
        return self.nodes[..., o:o + self.nnode[i]]
