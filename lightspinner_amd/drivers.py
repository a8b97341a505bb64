"""Driver loops of the reference, over an Engine / Context with many columns.

D1  test.py:20-29 / response_fn.py:11-21  -- MALI iteration to convergence
D2  response_fn.py:23-67                  -- brute-force temperature response function
D3  (no counterpart in the reference)     -- time steps of the rate equation, each iterated to consistency with the radiation
"""
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np


@dataclass
class MaliHistory:
    dJ: List[float] = field(default_factory=list)
    dPops: List[float] = field(default_factory=list)   # nan while only J is iterated
    converged: bool = False
    nonfinite: bool = False     # some monitor was NaN / inf on the way (the reference carries on silently)

    @property
    def n_iter(self):
        return len(self.dJ)


def iterate_mali(ctx, dJ_tol=2e-3, dPops_tol=1e-3, n_lambda_only=3, max_iter=500,
                 reduce_max: Optional[Callable[[float, float], tuple]] = None, log=None) -> MaliHistory:
    """`while dJ > 2e-3 or dPops > 1e-3` loop of test.py:20-29 with the reference's
    defaults: the first 3 iterations update J only (`if i > 3`, test.py:27).

    ctx needs formal_sol_gamma_matrices() and stat_equil() (Context or
    an Engine adapter).  reduce_max((dJ, dPops)) -> (dJ, dPops) is the hook where the
    multi-GPU driver takes the max over ranks (parallel.allreduce_max)."""
    h = MaliHistory()
    dJ, dPops, i = 1.0, 1.0, 0
    while dJ > dJ_tol or dPops > dPops_tol:
        i += 1
        dJ = ctx.formal_sol_gamma_matrices()
        if i > n_lambda_only:
            dPops = ctx.stat_equil()
        if reduce_max is not None:
            dJ, dPops = reduce_max(dJ, dPops)
        h.dJ.append(dJ)
        h.dPops.append(dPops if i > n_lambda_only else float('nan'))
        if log:
            log('Iteration %.3d: dJ: %.2e, dPops: %s' % (i, dJ, 'Just iterating Jbar' if i <= n_lambda_only else '%.2e' % dPops))
        if not (np.isfinite(dJ) and np.isfinite(dPops)):
            h.nonfinite = True          # the loop condition decides, exactly as in the reference: NaN > tol is False
        if i >= max_iter:
            break
    h.converged = (dJ <= dJ_tol and dPops <= dPops_tol)
    return h


def mali_step(engine, with_stat_equil=True, reducer=None):
    """One MALI iteration over every column of `engine` (problem.Engine): both calls are enqueued, then the
    convergence monitors are read ONCE -- lsx_sync on one rank, or reducer.engine(engine) over several (parallel.
    MaxReducer: the monitors stay on the device until the all-reduce has run).  -> (dJ, dPops or None)"""
    engine.formal_sol_gamma_async()
    if with_stat_equil:
        engine.stat_equil_async()
    if reducer is not None:
        dJ, dP = reducer.engine(engine)
    else:
        dJ, dP = engine.sync()
    return dJ, (dP if with_stat_equil else None)


def _begin(engine, reducer):
    if reducer is not None:
        reducer.engine_begin(engine)
    else:
        engine.sync_begin()


def _end(engine, reducer):
    return reducer.engine_end(engine) if reducer is not None else engine.sync_end()


def mali_steps(engine, nsteps, reducer=None, n_lambda_only=0, first=1, lookahead=None):
    """`nsteps` MALI iterations, yielding (dJ, dPops or None) after each, WITHOUT a host round trip between them: the next
    iteration's formal solution is enqueued before the monitors of the current one are waited for (include/lsx.h, lsx_sync_begin /
    lsx_sync_end), so the GPU goes from one iteration into the next while the host reads.  The iterations are numbered from
    `first`; those with a number > n_lambda_only include stat_equil (test.py:27).  The caller consumes every step (no early
    exit: nothing is rolled back here -- iterate_mali_engine does that).  lookahead (default: lsx_prefers_lookahead) False: the plain
    sequence of mali_step calls."""
    if nsteps < 1:
        return
    if lookahead is None:
        lookahead = engine.prefers_lookahead()
    if not lookahead:
        for s in range(nsteps):
            yield mali_step(engine, first + s > n_lambda_only, reducer)
        return
    i = first
    engine.formal_sol_gamma_async()
    se = i > n_lambda_only
    if se:
        engine.stat_equil_async()
    _begin(engine, reducer)
    for s in range(nsteps):
        last = s == nsteps - 1
        if not last:
            engine.formal_sol_gamma_async()            # iteration i + 1: nothing to take back, so the plain call
        dJ, dP = _end(engine, reducer)
        yield dJ, (dP if se else None)
        if not last:
            i += 1
            se = i > n_lambda_only
            if se:
                engine.stat_equil_async()
            _begin(engine, reducer)


def iterate_mali_engine(engine, reducer=None, dJ_tol=2e-3, dPops_tol=1e-3, n_lambda_only=3, max_iter=500, log=None,
                        pipelined=None) -> MaliHistory:
    """iterate_mali (test.py:20-29) on an Engine with many columns, globally converged: the loop runs until the maxima
    over all columns (and, with a reducer, over all ranks) are below the thresholds.

    pipelined (default: where the library says it pays, lsx_prefers_lookahead -- small contexts, e.g. a single column): iteration
    i + 1's formal solution is enqueued speculatively before the monitors of iteration i are known and discarded if the loop ends
    there (lsx_formal_sol_gamma_speculative / lsx_discard_formal_sol) -- the same iterations, the same results bit for bit, no
    idle GPU between iterations."""
    h = MaliHistory()
    if pipelined is None:
        pipelined = engine.prefers_lookahead()
    if max_iter < 1:
        return h

    def record(i, dJ, dPops):
        h.dJ.append(dJ)
        h.dPops.append(dPops if i > n_lambda_only else float('nan'))
        if log:
            log('Iteration %.3d: dJ: %.2e, dPops: %s' % (i, dJ, 'Just iterating Jbar' if i <= n_lambda_only else '%.2e' % dPops))
        if not (np.isfinite(dJ) and np.isfinite(dPops)):
            h.nonfinite = True

    dJ, dPops, i = 1.0, 1.0, 0
    if not pipelined:
        while dJ > dJ_tol or dPops > dPops_tol:
            i += 1
            dJ, dP = mali_step(engine, i > n_lambda_only, reducer)
            if dP is not None:
                dPops = dP
            record(i, dJ, dPops)
            if i >= max_iter:
                break
        h.converged = (dJ <= dJ_tol and dPops <= dPops_tol)
        return h

    i = 1
    engine.formal_sol_gamma_async()
    if i > n_lambda_only:
        engine.stat_equil_async()
    _begin(engine, reducer)
    can_speculate = True
    while True:
        speculating = can_speculate and i < max_iter
        if speculating:
            try:
                engine.formal_sol_gamma_speculative()          # iteration i + 1, ahead of the decision
            except Exception as e:
                from ._capi import LSX_EUNSUPPORTED
                if getattr(e, 'code', None) != LSX_EUNSUPPORTED:
                    # a failed enqueue: collect the read-back in flight, take back whatever part of the call was enqueued
                    # (the library has already switched buffers), and let the caller see the error
                    try:
                        _end(engine, reducer)
                    finally:
                        try:
                            engine.discard_formal_sol()
                        except Exception:
                            pass
                    raise
                # LSX_EUNSUPPORTED is the library's refusal BEFORE anything is enqueued (frozen columns): the loop goes on
                # without looking ahead
                can_speculate = speculating = False
        try:
            dJ, dP = _end(engine, reducer)                      # monitors of iteration i
        except Exception:
            if speculating:
                engine.discard_formal_sol()
            raise
        if i > n_lambda_only:
            dPops = dP
        record(i, dJ, dPops)
        if not (dJ > dJ_tol or dPops > dPops_tol) or i >= max_iter:
            if speculating:
                engine.discard_formal_sol()                     # the loop ends with iteration i: its I, J, Gamma are the results
            break
        i += 1
        if not speculating:
            engine.formal_sol_gamma_async()
        if i > n_lambda_only:
            engine.stat_equil_async()
        _begin(engine, reducer)
    h.converged = (dJ <= dJ_tol and dPops <= dPops_tol)
    return h


def response_function(I_plus, I_minus, I_base, mu_index=-1):
    """response_fn.py:59-67: rf[la, k] = (I+[la, mu] - I-[la, mu]) / I_base[la, mu].
    I_plus / I_minus: [Nspace][Nspect][Nrays] (one converged run per perturbed depth),
    I_base: [Nspect][Nrays]."""
    Ip = np.asarray(I_plus)[:, :, mu_index].T      # [Nspect][Nspace]
    Im = np.asarray(I_minus)[:, :, mu_index].T
    return (Ip - Im) / np.asarray(I_base)[:, mu_index][:, None]


def iterate_mali_columns(engine, dJ_tol=2e-3, dPops_tol=1e-3, n_lambda_only=3, max_iter=500, all_done=None, log=None,
                         report=None):
    """Many independent columns, each with the reference's own stopping rule: a column is frozen
    (lsx_set_active_columns) as soon as ITS dJ <= 2e-3 and dPops <= 1e-3, so it performs exactly the
    iterations a single-column reference Context would (test.py:20-29, response_fn.py:11-21).

    engine: problem.Engine.  all_done(bool) -> bool: hook for the multi-GPU driver (logical AND over
    ranks).  Returns the number of iterations each column took ([ncol] int array).

    A column whose monitors turn NaN is treated as the reference's `while dJ > 2e-3 or dPops > 1e-3` treats it: the
    comparisons with NaN are False, so the column stops as soon as its other monitor is below its threshold (it does
    not keep the batch iterating to max_iter).  report (a dict, optional) receives 'nonfinite': the indices of the
    columns that ever showed a non-finite monitor."""
    from . import _capi
    ncol = engine.ncol
    active = np.ones(ncol, dtype=bool)
    dP = np.ones(ncol)
    n_iter = np.zeros(ncol, dtype=np.int64)
    bad = np.zeros(ncol, dtype=bool)
    i = 0
    engine.set_active_columns(None)
    while True:
        i += 1
        engine.formal_sol_gamma()
        dJ = engine.get(_capi.LSX_DJ_COL)
        if i > n_lambda_only:
            engine.stat_equil()
            dP = np.where(active, engine.get(_capi.LSX_DPOPS_COL), dP)
        n_iter[active] = i
        bad |= active & ~(np.isfinite(dJ) & np.isfinite(dP))
        with np.errstate(invalid='ignore'):
            still = (dJ > dJ_tol) | (dP > dPops_tol)      # NaN compares False (test.py:23)
        active &= still
        if i >= max_iter:
            active[:] = False
        done = not active.any()
        if all_done is not None:
            done = all_done(done)
        if log:
            log('Iteration %.3d: %d of %d columns still iterating' % (i, int(active.sum()), ncol))
        if done:
            break
        engine.set_active_columns(active)
    engine.set_active_columns(None)
    if report is not None:
        report['nonfinite'] = np.flatnonzero(bad)
    return n_iter


def advance_time_columns(engine, dt, nsteps=1, dJ_tol=2e-3, dPops_tol=1e-3, max_iter=200, all_done=None, log=None):
    """`nsteps` time steps of the rate equation dn/dt = Gamma n for many independent columns (include/lsx_hip_timedep.h).  Per
    step, every column starts from its current populations (Engine.time_dep_start; dt: seconds, a scalar or one value per column);
    then formal solution + time_dep_update alternate until each column meets ITS tolerances, a column being frozen
    (lsx_set_active_columns) as soon as it does, as in iterate_mali_columns.  There are no Lambda-only iterations: the populations
    move from the first iteration on.  all_done(bool) -> bool: the multi-rank hook (logical AND over ranks), asked once per inner
    iteration.  -> the inner iterations each column took in each step ([nsteps][ncol] int array)."""
    from . import _capi
    ncol = engine.ncol
    counts = np.zeros((int(nsteps), ncol), dtype=np.int64)
    for step in range(int(nsteps)):
        engine.set_active_columns(None)
        engine.time_dep_start(dt)
        active = np.ones(ncol, dtype=bool)
        dP = np.ones(ncol)
        i = 0
        while True:
            i += 1
            engine.formal_sol_gamma()
            dJ = engine.get(_capi.LSX_DJ_COL)
            engine.time_dep_update()
            dP = np.where(active, engine.get(_capi.LSX_DPOPS_COL), dP)
            counts[step, active] = i
            with np.errstate(invalid='ignore'):
                still = (dJ > dJ_tol) | (dP > dPops_tol)      # NaN compares False, as in iterate_mali_columns
            active &= still
            if i >= max_iter:
                active[:] = False
            done = not active.any()
            if all_done is not None:
                done = all_done(done)
            if log:
                log('Step %d, iteration %.3d: %d of %d columns still iterating' % (step + 1, i, int(active.sum()), ncol))
            if done:
                break
            engine.set_active_columns(active)
        engine.set_active_columns(None)
    return counts


def fit_field_columns(backend, obs, mus, basis, nodes0, nnode, weight=None, base=None, lo=None, hi=None, lambda0=1e-2, factor=10.0,
                      lambda_min=1e-9, lambda_max=1e8, tol=1e-12, max_iter=30, log=None, penalty=None, uncertainty=False, scale=None,
                      **call):
    """Levenberg-Marquardt fit of the field vector of many independent columns to observed Stokes profiles (include/lsx_hip_fit.h).
    backend: anything with fit_field_normal, fit_field_chi2 and fit_field_step as Engine has them (an Engine is one).  obs
    [ncol][4][nla][nmu]; basis [P][Nspace], nnode, nodes0 [ncol][P], weight, base as in Engine.fit_field_normal; lo, hi [P]: bounds
    of the node values; **call: what else the backend's two field calls take (patterns, la0, nla, col0, ncol, amplitudes for the
    normal equations; instrument: a fit.Instrument, then obs and weight are [ncol][4][nobs][nmu]).  Per iteration and column: the normal equations at the nodes, the damped step, chi2 of the trial; where chi2
    fell the trial is accepted and lambda /= factor (not below lambda_min), otherwise lambda *= factor.  A column is done when a
    trial moved chi2 by less than tol x the chi2 the column started from (the trial is still accepted if it is lower), when lambda
    passes lambda_max, or at max_iter; a done column is frozen: its nodes no longer move.  This loop compares and scales scalars;
    every sum and every solve is the backend's.
    penalty: a fit.Penalty (include/lsx_hip_fit_regular.h): every normal-equation call and every chi2 call is followed by
    backend.fit_field_penalty, and the loop minimises data + penalty (.chi2, .history); .chi2_data and .penalty are the two parts.
    uncertainty=True: after the loop one more fit_field_normal at the final nodes, then backend.fit_field_uncertainty on the data's
    hess (with the penalty: the sandwich) -> .uncertainty.  scale: what the covariance is multiplied by -- None, [ncol], or 'reduced':
    chi2_data / (N - P) with N the column's points of positive weight (a column with N <= P has no estimate: NaN, status 1); a scale
    without uncertainty=True is refused.
    Without the two the backend sees the calls it ever saw.  -> fit.FieldFit."""
    from .fit import CONVERGED, LAMBDA_CEILING, MAX_ITER, FieldFit
    if isinstance(scale, str) and (scale != 'reduced' or obs is None):
        raise ValueError("fit_field_columns: scale is None, an array [ncol] or 'reduced' (which needs obs)")
    if scale is not None and not uncertainty:
        raise ValueError('fit_field_columns: scale multiplies the covariance: it goes with uncertainty=True')
    nodes = np.array(np.atleast_2d(np.asarray(nodes0, dtype=np.float64)), dtype=np.float64)
    ncol = nodes.shape[0]
    chi2_call = {k: v for k, v in call.items() if k != 'amplitudes'}
    lam = np.full(ncol, float(lambda0))
    active = np.ones(ncol, dtype=bool)
    status = np.full(ncol, MAX_ITER, dtype=np.int32)
    iterations = np.zeros(ncol, dtype=np.int64)
    chi2, field = backend.fit_field_chi2(mus, basis, nnode, nodes, obs, weight=weight, base=base, **chi2_call)
    chi2 = np.array(chi2, dtype=np.float64)
    chi2_data, pen = chi2, None
    if penalty is not None:
        chi2_data = chi2.copy()
        chi2, _, _, pen = backend.fit_field_penalty(nodes, penalty, chi2_data)
        chi2, pen = np.array(chi2, dtype=np.float64), np.array(pen, dtype=np.float64)
    first = chi2.copy()
    history = [chi2.copy()]
    for it in range(1, int(max_iter) + 1):
        if not active.any():
            break
        ne = backend.fit_field_normal(mus, basis, nnode, nodes, obs, weight=weight, base=base, **call)
        grad, hess = ne.grad, ne.hess
        if penalty is not None:
            _, grad, hess, _ = backend.fit_field_penalty(nodes, penalty, ne.chi2, ne.grad, ne.hess)
        trial, _, st = backend.fit_field_step(hess, grad, lam, nodes, lo, hi)
        trial = np.where(active[:, None], trial, nodes)               # a frozen column is asked about its own nodes
        c_trial, f_trial = backend.fit_field_chi2(mus, basis, nnode, trial, obs, weight=weight, base=base, **chi2_call)
        if penalty is not None:
            d_trial = np.array(c_trial, dtype=np.float64)
            c_trial, _, _, p_trial = backend.fit_field_penalty(trial, penalty, d_trial)
        with np.errstate(invalid='ignore'):
            accept = active & (st == 0) & (c_trial < chi2)
            settled = active & (st == 0) & (np.abs(c_trial - chi2) < tol * first)
        iterations[active] = it
        nodes[accept] = trial[accept]
        field[accept] = f_trial[accept]
        chi2[accept] = c_trial[accept]
        if penalty is not None:
            chi2_data[accept] = d_trial[accept]
            pen[accept] = p_trial[accept]
        lam = np.where(accept, np.maximum(lam / factor, lambda_min), np.where(active, lam * factor, lam))
        settled |= active & (chi2 == 0.0)
        ceiling = active & ~settled & (lam > lambda_max)
        status[settled] = CONVERGED
        status[ceiling] = LAMBDA_CEILING
        active &= ~(settled | ceiling)
        history.append(chi2.copy())
        if log:
            log('Fit iteration %.3d: %d of %d columns still iterating, largest chi2 %.6e' % (it, int(active.sum()), ncol, float(chi2.max())))
    # the degrees of freedom: a count of the points of positive weight, no sum over the data -- made when it is asked for (FieldFit.dof),
    # so that a fit without the new arguments does no more on the host than it ever did
    def count_dof():
        if obs is None:
            return None
        shape = np.shape(obs)
        if weight is None:
            return np.full(ncol, int(np.prod(shape[1:]))) - nodes.shape[1]
        try:
            positive = np.broadcast_to(np.asarray(weight), shape).reshape(ncol, -1) > 0
        except ValueError:                # a weight of another shape is the backend's to judge
            return None
        return np.count_nonzero(positive, axis=1) - nodes.shape[1]

    dof = count_dof
    unc = None
    if uncertainty:
        s = scale
        none = np.zeros(ncol, dtype=bool)
        if isinstance(scale, str):        # 'reduced'
            dof = count_dof()
            if dof is None:
                raise ValueError("fit_field_columns: scale='reduced' needs a weight of the shape of obs (or None)")
            none = dof <= 0
            s = np.where(none, 1.0, chi2_data / np.where(none, 1, dof))
        ne = backend.fit_field_normal(mus, basis, nnode, nodes, obs, weight=weight, base=base, **call)
        unc = backend.fit_field_uncertainty(ne.hess, basis, nnode, penalty=penalty, scale=s)
        if none.any():                    # no estimate of the scale: no uncertainty
            for a in (unc.ainv, unc.cov, unc.sigma, unc.field_sigma):
                if a is not None:
                    a[none] = np.nan
            unc.status[none] = 1
    return FieldFit(nodes, field, chi2, np.array(history), lam, iterations, status, nnode, penalty=pen, chi2_data=chi2_data,
                    uncertainty=unc, dof=dof)
