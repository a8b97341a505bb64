"""Ng acceleration of the MALI loop (include/lsx_hip_ng.h): the checker.

A numpy restatement of the scheme -- per column a counter and a history of order + 2 population vectors; per atom the weighted
normal equations of Ng (1974) / Olson, Auer & Buchler (1986) -- that drives ANY engine through Engine.get / set(LSX_N).  Over the
oracle it is the recorded expectation of the GPU tests (tests/test_ng.py); tests/test_ng_host.py pins it by exactness on
geometric sequences and by the iteration counts it was specified with."""
import functools

import mpmath
import numpy as np

from conftest import golden
from lightspinner_amd import _capi, fixtures
from lightspinner_amd.problem import Engine

U = 2.0 ** -53
MP = mpmath.mp.clone()
MP.dps = 50
K_COEF = 4          # coefficients_bar
DJ_TOL, DPOPS_TOL, N_LAMBDA_ONLY = 2e-3, 1e-3, 3          # the reference's loop (test.py:20-29)


# ---- the extrapolation of one atom ------------------------------------------------------------------------------------------
def normal_equations(xs, order):
    """xs: order + 2 vectors, NEWEST FIRST (x0, x1, ...), any shape -> (A [order][order], b [order])"""
    x = [np.asarray(v, dtype=np.float64).reshape(-1) for v in xs[:order + 2]]
    w = 1.0 / x[0] ** 2
    d0 = x[0] - x[1]
    D = [d0 - (x[j] - x[j + 1]) for j in range(1, order + 1)]
    A = np.array([[np.sum(w * D[i] * D[j]) for j in range(order)] for i in range(order)])
    b = np.array([np.sum(w * d0 * D[i]) for i in range(order)])
    return A, b


def combine(c, xs):
    """x_acc = (1 - sum c_j) x0 + sum c_j x_j"""
    out = (1.0 - np.sum(c)) * np.asarray(xs[0], dtype=np.float64)
    for j, cj in enumerate(c):
        out = out + cj * np.asarray(xs[j + 1], dtype=np.float64)
    return out


def extrapolate(xs, order):
    """-> (c [order], x_acc) or None where the system is not regular (singular, or not finite)"""
    A, b = normal_equations(xs, order)
    with np.errstate(all='ignore'):
        if not (np.all(np.isfinite(A)) and np.all(np.isfinite(b))):
            return None
        try:
            c = np.linalg.solve(A, b)
        except np.linalg.LinAlgError:
            return None
        if not np.all(np.isfinite(c)):
            return None
        return c, combine(c, xs)


# ---- the state machine of one column ----------------------------------------------------------------------------------------
class NgColumn:
    def __init__(self, prob, order, delay=0):
        self.prob, self.order, self.delay = prob, int(order), int(delay)
        self.applied = self.rejected = 0
        self.coef = np.zeros((prob.Natoms, 2))
        self.reset()

    def reset(self):
        self.cnt, self.hist = -self.delay, []

    @property
    def stored(self):
        return self.cnt

    def after_stat_equil(self, n):
        """n [NLtot][Nspace]: what the statistical equilibrium has just written.
        -> None (nothing to write back) or (x_acc [NLtot][Nspace], dPops of the column)"""
        if self.cnt < 0:
            self.cnt += 1
            return None
        self.hist.insert(0, np.array(n, dtype=np.float64))
        self.cnt += 1
        if self.cnt < self.order + 2:
            return None
        xs, p = self.hist, self.prob
        self.reset_history()
        out, coef = np.empty_like(xs[0]), np.zeros_like(self.coef)
        for a in range(p.Natoms):
            sl = slice(p.lev_off[a], p.lev_off[a] + p.Nlevel[a])
            r = extrapolate([x[sl] for x in xs], self.order)
            if r is None:
                self.rejected += 1
                return None
            coef[a, :self.order] = r[0]
            out[sl] = r[1].reshape(out[sl].shape)
        if not (np.all(np.isfinite(out)) and np.all(out > 0)):
            self.rejected += 1
            return None
        self.applied += 1
        self.coef = coef
        with np.errstate(all='ignore'):
            return out, float(np.nanmax(np.abs(1.0 - xs[1] / out)))

    def reset_history(self):
        self.cnt, self.hist = 0, []


# ---- the MALI loop of one single-column engine, plain or with the restatement on top ----------------------------------------
class Run:
    def __init__(self):
        self.dJ, self.dPops, self.n, self.applied, self.rejected, self.converged = [], [], None, 0, 0, False

    @property
    def n_iter(self):
        return len(self.dJ)


def iterate(eng, ng=None, dJ_tol=DJ_TOL, dPops_tol=DPOPS_TOL, max_iter=400):
    """test.py:20-29 on a one-column engine; ng: an NgColumn applied behind every stat_equil through get / set(LSX_N)
    (None: the plain loop -- or an engine that accelerates itself).  -> Run"""
    r = Run()
    dJ, dP, i = 1.0, 1.0, 0
    while dJ > dJ_tol or dP > dPops_tol:
        i += 1
        dJ = eng.formal_sol_gamma()
        if i > N_LAMBDA_ONLY:
            dP = eng.stat_equil()
            if ng is not None:
                step = ng.after_stat_equil(eng.get(_capi.LSX_N)[0])
                if step is not None:
                    eng.set(_capi.LSX_N, step[0][None])
                    dP = step[1]
        r.dJ.append(dJ)
        r.dPops.append(dP if i > N_LAMBDA_ONLY else float('nan'))
        if i >= max_iter:
            break
    r.converged = dJ <= dJ_tol and dP <= dPops_tol
    r.n = eng.get(_capi.LSX_N)[0]
    if ng is not None:
        r.applied, r.rejected = ng.applied, ng.rejected
    return r


FIXTURES = {'ca': 'falc_ca.npz', 'cah': 'falc_cah.npz'}
# what the feature was specified with (CPU, the restatement over the oracle, the reference's thresholds, delay 0)
PLAIN_ITERATIONS = {'ca': 46, 'cah': 79}
NG_ITERATIONS = {('ca', 1): 35, ('ca', 2): 25, ('cah', 1): 72, ('cah', 2): 37}


@functools.lru_cache(maxsize=None)
def problem(case):
    return fixtures.load_problem_npz(golden(FIXTURES[case]))


_RUNS = {}


def oracle_run(oracle_lib, case, order=0, tight=False):
    """the loop over the oracle, computed once per session: order 0 plain, 1 / 2 the restatement on top; tight: thresholds 1e-8"""
    key = (case, order, tight)
    if key not in _RUNS:
        prob, block, _ = problem(case)
        e = Engine(prob, 1, lib=oracle_lib)
        e.set_columns(0, block)
        tol = dict(dJ_tol=1e-8, dPops_tol=1e-8) if tight else {}
        _RUNS[key] = iterate(e, NgColumn(prob, order) if order else None, **tol)
        e.close()
    return _RUNS[key]


def popdist(n, ref):
    """largest relative population difference"""
    return float(np.max(np.abs(n - ref) / np.abs(ref)))


# ---- exact arithmetic for the GPU tests --------------------------------------------------------------------------------------
def exact_coefficients(xs, order):
    """the normal equations formed and solved in 50 digits from the float64 history xs (newest first)
    -> (c [order] as float, cond_2(A) as float)"""
    x = [[MP.mpf(float(v)) for v in np.asarray(q, dtype=np.float64).reshape(-1)] for q in xs[:order + 2]]
    N = len(x[0])
    w = [1 / (x[0][e] * x[0][e]) for e in range(N)]
    d0 = [x[0][e] - x[1][e] for e in range(N)]
    D = [[d0[e] - (x[j][e] - x[j + 1][e]) for e in range(N)] for j in range(1, order + 1)]
    A = MP.matrix(order, order)
    b = MP.matrix(order, 1)
    for i in range(order):
        b[i] = MP.fsum(w[e] * d0[e] * D[i][e] for e in range(N))
        for j in range(order):
            A[i, j] = MP.fsum(w[e] * D[i][e] * D[j][e] for e in range(N))
    c = MP.lu_solve(A, b)
    sv = MP.svd_r(A, compute_uv=False)
    return np.array([float(c[i]) for i in range(order)]), float(max(sv) / min(sv))


def coefficients_bar(N, order, cond, c):
    """|c_device - c_exact| <= K (N + order) u cond_2(A) |c|_2, K = 4.  Why: x0 - x1 of neighbouring iterates is exact or rounds
    once, so every term w D_i D_j carries at most 8 roundings (x0 x0, the reciprocal, one per D, two products, D's own two
    differences) and a sum of N of them N more: the computed A and b are the exact ones of data perturbed by (N + 8) u normwise
    (the terms of A_ij and b_i are bounded by those of the diagonal, Cauchy-Schwarz), the solution of the order x order system
    moves by 2 cond times that, and its own elimination adds a few u cond.  4 (N + order) >= 2 (N + 8) + 8 from N = 6 on, the
    smallest case.  -> (absolute bar, the relative bound)"""
    rel = K_COEF * (N + order) * U * cond
    return rel * float(np.linalg.norm(c)), rel


def combination_excess(n_dev, c, xs):
    """|n_dev - ((1 - sum c) x0 + sum c_j x_j)|, the combination in 50 digits from the float64 c and xs (newest first), over the
    bar (order + 3) u (|1 - sum c| |x0| + sum |c_j| |x_j|): the weights' sum and difference, the products and the additions round
    once each at most (fewer where the device fuses a product into an addition) -> the largest ratio"""
    order = len(c)
    cm = [MP.mpf(float(v)) for v in c]
    s = 1 - MP.fsum(cm)
    x = [np.asarray(q, dtype=np.float64).reshape(-1) for q in xs[:order + 1]]
    nd = np.asarray(n_dev, dtype=np.float64).reshape(-1)
    worst = MP.mpf(0)
    for e in range(nd.size):
        v = [MP.mpf(float(q[e])) for q in x]
        exact = s * v[0] + MP.fsum(cm[j] * v[j + 1] for j in range(order))
        bar = (order + 3) * MP.mpf(U) * (abs(s) * abs(v[0]) + MP.fsum(abs(cm[j]) * abs(v[j + 1]) for j in range(order)))
        worst = max(worst, abs(MP.mpf(float(nd[e])) - exact) / bar)
    return float(worst)
