"""Bodies of the time-dependent tests (include/lsx_hip_timedep.h): one implicit step of the rate equation dn/dt = Gamma n per
column, atom and depth, shared by the CPU run on the host build of the formulas (tests/test_time_dependent_host.py, -m "not gpu")
and the GPU run on the HIP library (tests/test_time_dependent.py, -m gpu).

Gamma is steered as in tests/se_cases.py: a probe atom's LSX_GAMMA is the collisional rates the test chose, bit for bit.

The checker is written from the scheme alone.  Per system, with G the read-back LSX_GAMMA, n the iterate the call started from,
n_prev the populations at the start of the step and dt the column's time step:

    iE = argmax(n) (first maximum);  A[i][j] = delta_ij - dt G[i][j] for i != iE, formed exactly;  A[iE][:] = 1;
    b = n_prev,  b[iE] = the float64 sum of n_prev formed by a Python loop in level order;  x = A^-1 b, by mpmath at 50 digits.

Each population has the bar

    bar_i = 2 * 3 Nl u (|A^-1| P |L| |U| |x|)_i + 2 u (|A^-1| E |x|)_i,          u = 2^-53,
    E = I + dt |G| with row iE set to zero.

The first term is se_cases' elimination bound (Higham, Accuracy and Stability of Numerical Algorithms, Thm 9.4; L, U, P scipy's of
the float64 rounding of A).  The second covers forming delta - dt G in floating point: one rounding of the result (fma) or two
(product, then difference) perturb A[i][j] by at most 2 u (delta_ij + dt |G[i][j]|), and |dx| <= |A^-1| |dA| |x| to first order.
Row iE is ones, exactly: nothing is formed there, so its row of E is zero.  (With that row kept, the term would grow like
u dt |G| and make every check at dt x rate >= 1e11 vacuous; without it the bar is the smaller one.)
b carries no error: the kernel forms b[iE] by the same adds in the same order.  A bar wider than 1e-5 |x_i| would make the check
vacuous: asserted.  LSX_DPOPS_COL is checked as se_cases checks it, within max_i (|n / x|_i bar_i / |x_i| + 4 u (1 + |n / x|_i))."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg

import se_cases
from conftest import ROOT, golden
from se_cases import MP, NLS, ORDINARY, SHAPES, U, Worst, probe_problem, put, rates_of, start_populations
from lightspinner_amd import _capi, drivers, fixtures
from lightspinner_amd.problem import Engine
from toy import spec_problem

CSRC = os.path.join(ROOT, 'lightspinner_amd', 'csrc')
FAMILIES = {k: se_cases.FAMILIES[k] for k in ('rate_scale', 'wide_range', 'ties')}
DT0 = 1e-2          # dt[c] = DT0 10^c: with rates of 1e-6 ... 1e6 s^-1 inside one shape, dt x rate spans 1e-8 ... 1e8
N, G_, DP = _capi.LSX_N, _capi.LSX_GAMMA, _capi.LSX_DPOPS_COL
REDRAW_BAR = 2e-6   # a fifth of what the vacuity assertion accepts, as se_cases.wide_range


def column_dt(ncol, dt0=DT0):
    return dt0 * 10.0 ** np.arange(ncol)


# ---- the exact reference and its bars ---------------------------------------------------------------------------------------
def float_sum(v):
    s = 0.0
    for x in v:
        s = s + float(x)
    return s


_exact_cache = {}


def exact_step(G, n_prev, n_old, dt, rhs=None):
    """one system: G [Nl][Nl] read back, n_prev, n_old [Nl], dt -> (x as mpmath numbers, bar [Nl]).  rhs: what stands in for
    n_prev on the right-hand side (the deliberately wrong variant of the self-test)"""
    key = (G.tobytes(), np.asarray(n_prev).tobytes(), np.asarray(n_old).tobytes(), float(dt), None if rhs is None else np.asarray(rhs).tobytes())
    if key in _exact_cache:
        return _exact_cache[key]
    Nl = G.shape[0]
    iE = int(np.argmax(n_old))
    src = n_prev if rhs is None else rhs
    A = MP.matrix(Nl, Nl)
    mdt = MP.mpf(float(dt))
    for i in range(Nl):
        for j in range(Nl):
            A[i, j] = MP.mpf(1) if i == iE else (MP.mpf(1 if i == j else 0) - mdt * MP.mpf(float(G[i, j])))
    b = MP.matrix([MP.mpf(float(v)) for v in src])
    b[iE] = MP.mpf(float_sum(src))
    Ainv = MP.inverse(A)
    xm = Ainv * b
    x = [xm[i] for i in range(Nl)]
    absinv = np.array([[float(abs(Ainv[i, j])) for j in range(Nl)] for i in range(Nl)])
    Af = np.array([[float(A[i, j]) for j in range(Nl)] for i in range(Nl)])
    p, l, u = scipy.linalg.lu(Af)
    absx = np.array([float(abs(v)) for v in x])
    form = np.eye(Nl) + float(dt) * np.abs(np.asarray(G, dtype=np.float64))
    form[iE, :] = 0.0
    bar = 2.0 * 3.0 * Nl * U * (absinv @ (p @ (np.abs(l) @ np.abs(u))) @ absx) + 2.0 * U * (absinv @ form @ absx)
    _exact_cache[key] = (x, bar)
    return x, bar


def relative_bar_in_float64(Gm, n_prev, iE, dt):
    """the largest bar_i / |x_i| of the system, estimated in float64 from the inputs alone (the redraw criterion)"""
    Nl = Gm.shape[0]
    A = np.eye(Nl) - dt * Gm
    A[iE, :] = 1.0
    b = np.array(n_prev, dtype=np.float64)
    b[iE] = float_sum(n_prev)
    with np.errstate(all='ignore'):
        inv = np.linalg.inv(A)
        p, l, u = scipy.linalg.lu(A)
        x = np.abs(inv @ b)
        form = np.eye(Nl) + dt * np.abs(Gm)
        form[iE, :] = 0.0
        bar = 2.0 * 3.0 * Nl * U * (np.abs(inv) @ (p @ (np.abs(l) @ np.abs(u))) @ x) + 2.0 * U * (np.abs(inv) @ form @ x)
        r = float(np.max(bar / x))
    return r if r == r else np.inf


def gamma_of_rates(Ck):
    """Gamma of a probe atom in float64: the off-diagonals are the rates, the diagonal minus the column sum"""
    Gm = np.array(Ck, dtype=np.float64)
    np.fill_diagonal(Gm, 0.0)
    Gm[np.arange(len(Gm)), np.arange(len(Gm))] = -Gm.sum(0)
    return Gm


# ---- inputs -----------------------------------------------------------------------------------------------------------------
class Redraws:
    def __init__(self):
        self.systems, self.redrawn = 0, 0

    def check(self, tag=''):
        assert self.systems > 0
        share = self.redrawn / self.systems
        print('%s: %d of %d systems were drawn again' % (tag, self.redrawn, self.systems))
        assert share <= 0.10, '%s: %.1f %% of the systems were drawn again' % (tag, 100 * share)


def family_inputs(family, prob, block, a, seed, dt, redraws=None):
    """fill probe atom a of (prob, block) with systems of `family`: rates, the iterate n (in block.n) -> n_prev [ncol][Nl][Ns] of
    the atom.  The iterate has its maximum at the family's level; n_prev has its own at another level in a third of the systems.
    A system whose smallest population the bar would leave fewer than five digits of (estimated in float64 from the inputs) is
    drawn again as a whole; no system is skipped."""
    rng = np.random.default_rng(seed)
    Nl, Ns, nc = prob.Nlevel[a], prob.Nspace, block.ncol
    Cs, n, n_prev = np.zeros((nc, Nl, Nl, Ns)), np.zeros((nc, Nl, Ns)), np.zeros((nc, Nl, Ns))
    nTot = 1e14 * np.exp(9.0 * np.linspace(0.0, 1.0, Ns))[None, :] * 0.3 * (1.0 + 0.1 * np.arange(nc))[:, None]
    seen, moved = set(), 0
    for c in range(nc):
        for k in range(Ns):
            q = c * Ns + k
            first = True
            for attempt in range(1000):
                Ck, iE, tie = FAMILIES[family](rng, Nl, q)
                Ck[np.arange(Nl), np.arange(Nl)] = 0.0
                other = q % 9 in (0, 4, 8)       # a third of the systems, at every rate scale and every level of the iterate's maximum
                iP = (iE + 1) % Nl if other else iE
                prev = start_populations(rng, Nl, nTot[c, k], iP)
                it = start_populations(rng, Nl, nTot[c, k] * rng.uniform(0.9, 1.1), iE, tie)
                if relative_bar_in_float64(gamma_of_rates(Ck), prev, iE, dt[c]) <= REDRAW_BAR:
                    break
                first = False
            else:
                raise AssertionError('no acceptable draw for system %d of %s at dt = %g' % (q, family, dt[c]))
            if redraws is not None:
                redraws.systems += 1
                redraws.redrawn += 0 if first else 1
            Cs[c, :, :, k], n[c, :, k], n_prev[c, :, k] = Ck, it, prev
            seen.add(iE)
            moved += other
    assert 3 * moved >= nc * Ns
    put(prob, block, a, Cs, n, nTot)
    return n_prev, seen


def full_n_prev(prob, block, a, prev_a):
    """n_prev of every atom: the probe's as drawn, the others' a rescaled, reshuffled copy of their start"""
    out = np.array(block.n, dtype=np.float64)
    out *= 1.0 + 0.05 * np.cos(np.arange(out.size)).reshape(out.shape)
    o = prob.lev_off[a]
    out[:, o:o + prob.Nlevel[a]] = prev_a
    return out


# ---- the checker ------------------------------------------------------------------------------------------------------------
def check_step(w, prob, G, n_prev, n_old, n_new, dt, dPcol, singular=(), active=None, sums=None):
    """every system of every atom of every active column against the exact solve, LSX_DPOPS_COL, and (sums: a Worst-like dict)
    the number conservation: sum n_new against the float sum of n_prev within the sum of the components' bars"""
    ncol, Ns = G.shape[0], prob.Nspace
    for c in range(ncol):
        if active is not None and not active[c]:
            assert np.array_equal(n_new[c].view(np.uint64), n_old[c].view(np.uint64)), 'frozen column %d: populations changed' % c
            assert dPcol[c] == 0.0
            continue
        ch_max, ch_bar = 0.0, 0.0
        for a in range(prob.Natoms):
            Nl, o, o2 = prob.Nlevel[a], prob.lev_off[a], prob.lev2_off[a]
            Ga = G[c, o2:o2 + Nl * Nl].reshape(Nl, Nl, Ns)
            for k in range(Ns):
                old, new, prev = n_old[c, o:o + Nl, k], n_new[c, o:o + Nl, k], n_prev[c, o:o + Nl, k]
                if (c, a, k) in singular:
                    assert np.array_equal(old.view(np.uint64), new.view(np.uint64)), 'singular system %r: populations changed' % ((c, a, k),)
                    continue
                x, bar = exact_step(np.ascontiguousarray(Ga[:, :, k]), np.ascontiguousarray(prev), np.ascontiguousarray(old), dt[c])
                for i in range(Nl):
                    ax = float(abs(x[i]))
                    assert ax > 0.0 and bar[i] <= 1e-5 * ax, 'vacuous bar %.3g at %r' % (bar[i] / max(ax, 1e-300), (c, a, k, i))
                    w.relbar = max(w.relbar, bar[i] / ax)
                    dev = float(abs(MP.mpf(float(new[i])) - x[i]))
                    r = dev / bar[i]
                    w.pops[Nl] = max(w.pops.get(Nl, 0.0), r)
                    assert r <= 1.0, '%s: population at column %d, atom %d, depth %d, level %d: %.3g x the bar (%r, exact %s)' % (
                        w.tag, c, a, k, i, r, new[i], MP.nstr(x[i], 20))
                    q = float(abs(MP.mpf(float(old[i])) / x[i]))
                    ch_max = max(ch_max, float(abs(1 - MP.mpf(float(old[i])) / x[i])))
                    ch_bar = max(ch_bar, q * bar[i] / ax + 4.0 * U * (1.0 + q))
                if sums is not None:
                    # the exact x sums to b[iE] = the float sum of n_prev exactly (row iE); the computed sum adds the components'
                    # deviations and Nl - 1 roundings of numpy's own adds
                    tot = float_sum(prev)
                    got = float_sum(new)
                    sbar = float(np.sum(bar)) + (Nl - 1) * U * float(np.sum(np.abs(new)))
                    r = abs(got - tot) / sbar
                    sums['worst'] = max(sums.get('worst', 0.0), r)
                    assert r <= 1.0, '%s: number density at %r: %r against %r, %.3g x the bar' % (w.tag, (c, a, k), got, tot, r)
        r = abs(dPcol[c] - ch_max) / ch_bar
        w.mon = max(w.mon, r)
        assert r <= 1.0, '%s: DPOPS_COL[%d] = %r, exact %r: %.3g x the bar' % (w.tag, c, dPcol[c], ch_max, r)


# ---- runners: the HIP library on a GPU, or the oracle's Gamma through the host build of the formulas ---------------------
class HostLib:
    """liblsx_td_host.so (make tdhost): lsx_solve_dev.h compiled for the CPU, the time-dependent step and the statistical equilibrium"""
    def __init__(self):
        subprocess.check_call(['make', '-s', '-C', CSRC, 'tdhost'])
        self.dll = C.CDLL(os.path.join(CSRC, 'liblsx_td_host.so'))
        dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        self.dll.lsx_timedep_host.argtypes = [C.c_int32, C.c_int32, C.c_int32, dp, dp, dp, dp, dp, bp, bp, C.c_int32, C.c_int32]
        self.dll.lsx_timedep_host.restype = C.c_int
        self.dll.lsx_statequil_host.argtypes = [C.c_int32, C.c_int32, C.c_int32, dp, dp, dp, dp, bp, bp, C.c_int32, C.c_int32]
        self.dll.lsx_statequil_host.restype = C.c_int

    def solve(self, prob, G, nTotal, n_old, active=None, in_memory=False, work_stride=1):
        """the statistical equilibrium of every atom of every column -> (n_new, DPOPS_COL, {(col, atom, depth)} flagged)"""
        dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        ncol, Ns = G.shape[0], prob.Nspace
        n_new, dPcol, flagged = np.array(n_old), np.zeros(ncol), set()
        act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
        for a in range(prob.Natoms):
            Nl, o, o2 = prob.Nlevel[a], prob.lev_off[a], prob.lev2_off[a]
            Ga, na = np.ascontiguousarray(G[:, o2:o2 + Nl * Nl]), np.ascontiguousarray(n_old[:, o:o + Nl])
            nt, dP, sing = np.ascontiguousarray(nTotal[:, a], dtype=np.float64), np.zeros(ncol), np.zeros((ncol, Ns), dtype=np.uint8)
            rc = self.dll.lsx_statequil_host(Nl, Ns, ncol, Ga.ctypes.data_as(dp), nt.ctypes.data_as(dp), na.ctypes.data_as(dp),
                                             dP.ctypes.data_as(dp), sing.ctypes.data_as(bp),
                                             None if act is None else act.ctypes.data_as(bp), int(in_memory), int(work_stride))
            assert rc == 0
            n_new[:, o:o + Nl] = na
            dPcol = np.maximum(dPcol, dP)
            flagged |= {(int(c), a, int(k)) for c, k in zip(*np.nonzero(sing))}
        return n_new, dPcol, flagged

    def step(self, prob, G, n_prev, n_old, dt, active=None, in_memory=False, work_stride=1):
        """every atom of every column -> (n_new, DPOPS_COL, {(col, atom, depth)} flagged)"""
        dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        ncol, Ns = G.shape[0], prob.Nspace
        n_new, dPcol, flagged = np.array(n_old), np.zeros(ncol), set()
        act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
        for a in range(prob.Natoms):
            Nl, o, o2 = prob.Nlevel[a], prob.lev_off[a], prob.lev2_off[a]
            Ga = np.ascontiguousarray(G[:, o2:o2 + Nl * Nl])
            pa, na = np.ascontiguousarray(n_prev[:, o:o + Nl]), np.ascontiguousarray(n_old[:, o:o + Nl])
            dts, dP, sing = np.ascontiguousarray(dt, dtype=np.float64), np.zeros(ncol), np.zeros((ncol, Ns), dtype=np.uint8)
            rc = self.dll.lsx_timedep_host(Nl, Ns, ncol, Ga.ctypes.data_as(dp), pa.ctypes.data_as(dp), dts.ctypes.data_as(dp),
                                           na.ctypes.data_as(dp), dP.ctypes.data_as(dp), sing.ctypes.data_as(bp),
                                           None if act is None else act.ctypes.data_as(bp), int(in_memory), int(work_stride))
            assert rc == 0
            n_new[:, o:o + Nl] = na
            dPcol = np.maximum(dPcol, dP)
            flagged |= {(int(c), a, int(k)) for c, k in zip(*np.nonzero(sing))}
        return n_new, dPcol, flagged


class HostRunner:
    """Gamma from the oracle's formal solution (a CPU library), the step from the host build"""
    backend = 'host'

    def __init__(self, oracle_lib, host, in_memory=False):
        self.oracle, self.host, self.in_memory = oracle_lib, host, in_memory

    def __call__(self, prob, block, dt, n_prev, calls='sync'):
        e = Engine(prob, block.ncol, lib=self.oracle)
        e.set_columns(0, block)
        e.formal_sol_gamma()
        G, n_old = e.get(G_), e.get(N)
        e.close()
        n_new, dPcol, flagged = self.host.step(prob, G, n_prev, n_old, dt, in_memory=self.in_memory)
        assert not flagged
        return G, n_old, n_new, dPcol


class HipRunner:
    def __init__(self, lib, options=None):
        self.lib, self.options, self.backend = lib, options, lib.backend

    def __call__(self, prob, block, dt, n_prev, calls='sync'):
        e = Engine(prob, block.ncol, lib=self.lib, options=self.options)
        e.set_columns(0, block)
        e.formal_sol_gamma()
        G, n_old = e.get(G_), e.get(N)
        e.time_dep_start(dt, n_prev)
        if calls == 'sync':
            dP = e.time_dep_update()
            n_new = e.get(N)
        else:
            e.time_dep_update_async()
            e.sync_begin(populations=True)
            dP = e.sync_end()[1]
            n_new = e.fetch_populations()
            assert np.array_equal(n_new.view(np.uint64), e.get(N).view(np.uint64))
        dPcol = e.get(DP)
        assert dP == dPcol.max()
        e.close()
        return G, n_old, n_new, dPcol


# ---- 1, 4: the families ---------------------------------------------------------------------------------------------------------
def family(runner, name, Nl, calls=('sync',), results=None):
    """one family at one size on both context shapes; every call sequence of `calls` must give the same bits"""
    w = Worst('%s %s Nl=%d' % (runner.backend, name, Nl))
    red, sums, seen = Redraws(), {}, set()
    for s, (Ns, nc) in enumerate(SHAPES):
        prob, block, (a,) = probe_problem([Nl], Ns, nc)
        dt = column_dt(nc)
        prev_a, sn = family_inputs(name, prob, block, a, 7000 + 1000 * Nl + s, dt, red)
        seen |= sn
        n_prev = full_n_prev(prob, block, a, prev_a)
        out = [runner(prob, block, dt, n_prev, calls=c) for c in calls]
        for G, n_old, n_new, dPcol in out:
            check_step(w, prob, G, n_prev, n_old, n_new, dt, dPcol, sums=sums)
            assert np.array_equal(n_new.view(np.uint64), out[0][2].view(np.uint64))
            assert np.array_equal(dPcol.view(np.uint64), out[0][3].view(np.uint64))
        assert np.array_equal(block.n, out[0][1])
        if results is not None:
            results[(name, Nl, s)] = out[0]
    assert seen == {0, Nl // 2, Nl - 1}
    red.check(w.tag)
    w.report()
    print('%s: number conservation, worst deviation / bar: %.3g' % (w.tag, sums['worst']))
    return w


# ---- the checker pins itself --------------------------------------------------------------------------------------------------
def closed_form_two_levels():
    """n_1' = (n_1 + dt C_10 N) / (1 + dt (C_01 + C_10)), N = n_0 + n_1, for either eliminated row"""
    rng = np.random.default_rng(11)
    for q in range(60):
        C01, C10 = 10.0 ** rng.uniform(-6, 6, 2)          # C_ij: the rate j -> i
        dt = 10.0 ** rng.uniform(-6, 6)
        prev = 10.0 ** rng.uniform(10, 14, 2)
        old = 10.0 ** rng.uniform(10, 14, 2)
        G = np.array([[-C10, C01], [C10, -C01]])
        x, bar = exact_step(G, prev, old, dt)
        Nt = MP.mpf(float_sum(prev))
        d = 1 + MP.mpf(dt) * (MP.mpf(C01) + MP.mpf(C10))
        want1 = (MP.mpf(prev[1]) + MP.mpf(dt) * MP.mpf(C10) * Nt) / d
        want0 = (MP.mpf(prev[0]) + MP.mpf(dt) * MP.mpf(C01) * Nt) / d
        # (n_0 + n_1 = N holds for the exact sum; b[iE] is the float64 sum: the two agree within u N)
        for got, want in ((x[0], want0), (x[1], want1)):
            assert abs(got - want) <= 2 * U * Nt, (q, got, want)
        assert np.all(bar <= 1e-5 * np.array([float(v) for v in x]))


def wrong_variant_misses_its_bar(runner):
    """the checker with n_old in the place of n_prev on the right-hand side disagrees with what the scheme gives by far more
    than its bar: a confusion of the two arrays cannot pass"""
    Nl = 4
    Ns, nc = SHAPES[0]
    prob, block, (a,) = probe_problem([Nl], Ns, nc)
    dt = column_dt(nc)
    prev_a, _ = family_inputs('rate_scale', prob, block, a, 31, dt)
    n_prev = full_n_prev(prob, block, a, prev_a)
    G, n_old, n_new, dPcol = runner(prob, block, dt, n_prev)
    o, o2 = prob.lev_off[a], prob.lev2_off[a]
    missed = 0
    for c in range(nc):
        for k in range(Ns):
            Gk = np.ascontiguousarray(G[c, o2:o2 + Nl * Nl].reshape(Nl, Nl, Ns)[:, :, k])
            x, bar = exact_step(Gk, n_prev[c, o:o + Nl, k], n_old[c, o:o + Nl, k], dt[c], rhs=n_old[c, o:o + Nl, k])
            dev = max(float(abs(MP.mpf(float(n_new[c, o + i, k])) - x[i])) / bar[i] for i in range(Nl))
            missed += dev > 1.0
    assert missed == nc * Ns, missed


# ---- GPU bodies -----------------------------------------------------------------------------------------------------------------
def probe_engine(lib, Nl, shape=1, family_name='rate_scale', seed=5, options=None, dt=None):
    Ns, nc = SHAPES[shape]
    prob, block, (a,) = probe_problem([Nl], Ns, nc)
    dt = column_dt(nc) if dt is None else dt
    prev_a, _ = family_inputs(family_name, prob, block, a, seed, dt)
    n_prev = full_n_prev(prob, block, a, prev_a)
    e = Engine(prob, nc, lib=lib, options=options)
    e.set_columns(0, block)
    return e, prob, block, a, dt, n_prev


def instances_agree(lib, Nl):
    """se_lds=1 (the LDS kernel for every size) gives the bits of the register instance"""
    for name in FAMILIES:
        Ns, nc = SHAPES[1]
        prob, block, (a,) = probe_problem([Nl], Ns, nc)
        dt = column_dt(nc)
        prev_a, _ = family_inputs(name, prob, block, a, 90 + Nl, dt)
        n_prev = full_n_prev(prob, block, a, prev_a)
        out = [HipRunner(lib, options)(prob, block, dt, n_prev) for options in (None, 'se_lds=1')]
        assert np.array_equal(out[0][2].view(np.uint64), out[1][2].view(np.uint64)), (name, Nl)
        assert np.array_equal(out[0][3].view(np.uint64), out[1][3].view(np.uint64)), (name, Nl)
        assert not np.array_equal(out[0][2], out[0][1])


def limits(lib, Nl):
    """dt x min(rate) >= 1e12: the statistical equilibrium on the same Gamma with nTotal = sum n_prev; dt x max(rate) <= 1e-20:
    n_prev.  Each within the sum of both calls' bars.  (The exact solutions of the two systems differ by O(1 / (dt x rate)); the
    step is 1e40 s on rates >= 3e-8 s^-1 so that this is far below both bars, which are of the order of u.)"""
    Ns, nc = SHAPES[1]
    w = Worst('%s limits Nl=%d' % (lib.backend, Nl))
    for dtv, what in ((1e40, 'long'), (1e-28, 'short')):
        dt = np.full(nc, dtv)
        prob, block, (a,) = probe_problem([Nl], Ns, nc)
        prev_a, _ = family_inputs('rate_scale', prob, block, a, 300 + Nl, dt)
        rates = rates_of(prob, block.C, a)
        off = rates[rates > 0]
        assert dtv * off.min() >= 1e12 if what == 'long' else dtv * off.max() <= 1e-20
        n_prev = full_n_prev(prob, block, a, prev_a)
        G, n_old, n_new, dPcol = HipRunner(lib)(prob, block, dt, n_prev)
        check_step(w, prob, G, n_prev, n_old, n_new, dt, dPcol)
        o, o2 = prob.lev_off[a], prob.lev2_off[a]
        if what == 'long':
            nTot = np.array(block.nTotal)
            for c in range(nc):
                for k in range(Ns):
                    nTot[c, a, k] = float_sum(prev_a[c, :, k])
            put(prob, block, a, nTotal=nTot[:, a])
            e, G2, n_old2, n_se, dPcol2, dP2 = se_cases.run(lib, prob, block)
            e.close()
            assert np.array_equal(G, G2) and np.array_equal(n_old, n_old2)
        for c in range(nc):
            for k in range(Ns):
                Gk = np.ascontiguousarray(G[c, o2:o2 + Nl * Nl].reshape(Nl, Nl, Ns)[:, :, k])
                x, bar = exact_step(Gk, np.ascontiguousarray(n_prev[c, o:o + Nl, k]), np.ascontiguousarray(n_old[c, o:o + Nl, k]), dt[c])
                if what == 'long':
                    x2, bar2, _ = se_cases.exact_system(Gk, n_old[c, o:o + Nl, k], block.nTotal[c, a, k])
                    other, both = n_se[c, o:o + Nl, k], bar + bar2
                else:
                    other, both = n_prev[c, o:o + Nl, k], bar
                assert np.all(np.abs(n_new[c, o:o + Nl, k] - other) <= both), (what, c, k, n_new[c, o:o + Nl, k], other, both)
    w.report()


def second_update_from_another_iterate(lib, Nl):
    """the same Gamma, the same n_prev, another iterate: the same n_new within both bars -- only iE and the monitor differ"""
    e, prob, block, a, dt, n_prev = probe_engine(lib, Nl, seed=50 + Nl)
    w = Worst('%s second update Nl=%d' % (lib.backend, Nl))
    e.formal_sol_gamma()
    G, n0 = e.get(G_), e.get(N)
    e.time_dep_start(dt, n_prev)
    e.time_dep_update()
    n1, dP1 = e.get(N), e.get(DP)
    check_step(w, prob, G, n_prev, n0, n1, dt, dP1)
    e.time_dep_update()                          # no formal solution in between: the same Gamma, the iterate is now n1
    n2, dP2 = e.get(N), e.get(DP)
    assert np.array_equal(e.get(G_), G)
    check_step(w, prob, G, n_prev, n1, n2, dt, dP2)
    Ns = prob.Nspace
    ies = 0
    for c in range(block.ncol):
        for at in range(prob.Natoms):
            Nla, o, o2 = prob.Nlevel[at], prob.lev_off[at], prob.lev2_off[at]
            for k in range(Ns):
                Gk = np.ascontiguousarray(G[c, o2:o2 + Nla * Nla].reshape(Nla, Nla, Ns)[:, :, k])
                prev = np.ascontiguousarray(n_prev[c, o:o + Nla, k])
                _, b1 = exact_step(Gk, prev, np.ascontiguousarray(n0[c, o:o + Nla, k]), dt[c])
                _, b2 = exact_step(Gk, prev, np.ascontiguousarray(n1[c, o:o + Nla, k]), dt[c])
                assert np.all(np.abs(n2[c, o:o + Nla, k] - n1[c, o:o + Nla, k]) <= b1 + b2), (c, at, k)
                ies += int(np.argmax(n0[c, o:o + Nla, k])) != int(np.argmax(n1[c, o:o + Nla, k]))
    assert ies > 0                               # the eliminated row did move somewhere
    assert np.all(dP2 < dP1)
    e.close()
    w.report()


def frozen_columns(lib):
    Nl = 5
    e, prob, block, a, dt, n_prev = probe_engine(lib, Nl, seed=60)
    nc = block.ncol
    w = Worst('%s frozen' % lib.backend)
    e.formal_sol_gamma()
    G, n0 = e.get(G_), e.get(N)
    # a step on columns 1 ... 3 only; column 0 active: refused, nothing launched
    e.time_dep_start(dt[1:4], n_prev[1:4], col0=1, ncol=3)
    with pytest.raises(_capi.LsxError, match='column 0') as ei:
        e.time_dep_update()
    assert ei.value.code == _capi.LSX_EINVAL
    with pytest.raises(_capi.LsxError, match='column 0'):
        e.time_dep_update_async()
    assert np.array_equal(e.get(N).view(np.uint64), n0.view(np.uint64))
    active = np.zeros(nc, dtype=bool)
    active[1:4] = True
    e.set_active_columns(active)
    dP = e.time_dep_update()
    n1, dPcol = e.get(N), e.get(DP)
    full = np.where(active[:, None, None], n_prev, 0.0)
    st_dt, st_prev = e.time_dep_state()
    assert np.array_equal(st_dt, np.where(active, dt, 0.0))
    assert np.array_equal(st_prev.view(np.uint64), full.view(np.uint64))         # n_prev of every column as before the update
    check_step(w, prob, G, n_prev, n0, n1, dt, dPcol, active=active)
    assert dP == dPcol.max() and dPcol[0] == 0.0 and dPcol[4] == 0.0
    e.set_active_columns(None)
    with pytest.raises(_capi.LsxError, match='column 0'):
        e.time_dep_update()
    e.close()
    w.report()


def one_bad_system(lib, calls, Nl):
    """one NaN rate among regular systems: flagged and named as lsx_stat_equil names it, its populations untouched, the others
    correct (the pattern of se_cases.one_singular_system / nan_in_the_rates)"""
    Ns, nc = SHAPES[1]
    sc, sk = 3, 12
    prob, block, (a,) = probe_problem([Nl], Ns, nc)
    dt = column_dt(nc)
    prev_a, _ = family_inputs('rate_scale', prob, block, a, 70 + Nl, dt)
    n_prev = full_n_prev(prob, block, a, prev_a)
    bad = rates_of(prob, block.C, a).copy()
    bad[sc, Nl - 1, 0, sk] = np.nan
    put(prob, block, a, C=bad)
    w = Worst('%s one NaN rate (%s) Nl=%d' % (lib.backend, calls, Nl))
    e = Engine(prob, nc, lib=lib)
    e.set_columns(0, block)
    e.formal_sol_gamma()
    G, n0 = e.get(G_), e.get(N)
    e.time_dep_start(dt, n_prev)
    with pytest.raises(_capi.LsxSingularError, match=r'column %d, depth %d, atom %d\b' % (sc, sk, a)) as ei:
        if calls == 'sync':
            e.time_dep_update()
        else:
            e.time_dep_update_async()
            e.formal_sol_gamma_async()
            e.sync()
    assert ei.value.code == _capi.LSX_ESINGULAR
    check_step(w, prob, G, n_prev, n0, e.get(N), dt, e.get(DP), singular={(sc, a, sk)})
    e.close()
    w.report()


def refusals(lib):
    e, prob, block, a, dt, n_prev = probe_engine(lib, 4, shape=0, seed=80)
    nc = block.ncol

    def unchanged(want_dt, want_prev):
        st_dt, st_prev = e.time_dep_state()
        assert np.array_equal(st_dt, want_dt) and np.array_equal(st_prev.view(np.uint64), want_prev.view(np.uint64))

    def refused(call, *args, **kw):
        with pytest.raises(_capi.LsxError) as ei:
            call(*args, **kw)
        assert ei.value.code == _capi.LSX_EINVAL, ei.value

    e.formal_sol_gamma()
    n0 = e.get(N)
    zero = (np.zeros(nc), np.zeros_like(n_prev))
    unchanged(*zero)
    refused(e.time_dep_update)                   # an update before any start
    refused(e.time_dep_update_async)
    unchanged(*zero)
    assert np.array_equal(e.get(N).view(np.uint64), n0.view(np.uint64))
    for state in (zero, (dt, n_prev)):
        for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
            d = dt.copy()
            d[1] = bad
            refused(e.time_dep_start, d, n_prev)
            refused(e.time_dep_start, d)
            refused(e.time_dep_start, bad)
            unchanged(*state)
        for col0, ncol in ((-1, 2), (0, 0), (0, nc + 1), (nc, 1), (2, nc - 1), (0, -1)):
            refused(e.time_dep_start, 1.0, None, col0, ncol)
            with pytest.raises(_capi.LsxError) as ei:
                e.time_dep_state(col0, ncol)
            assert ei.value.code == _capi.LSX_EINVAL
            unchanged(*state)
        with pytest.raises(_capi.LsxError) as ei:      # a null dt, straight at the entry
            lib.check(lib.dll.lsx_hip_time_dep_start(e._h, 0, nc, None, None))
        assert ei.value.code == _capi.LSX_EINVAL
        unchanged(*state)
        if state is zero:
            e.time_dep_start(dt, n_prev)
    e.time_dep_update()                          # and the engine goes on
    e.close()


def state_round_trip(lib):
    e, prob, block, a, dt, n_prev = probe_engine(lib, 9, seed=81)
    e.time_dep_start(dt, n_prev)
    st_dt, st_prev = e.time_dep_state()
    assert np.array_equal(st_dt, dt) and np.array_equal(st_prev.view(np.uint64), n_prev.view(np.uint64))
    # a sub-range, the snapshot form: the populations as they are on the device, bit for bit; the rest keeps what it had
    e.formal_sol_gamma()
    e.time_dep_update()
    now = e.get(N)
    e.time_dep_start(2.5, col0=1, ncol=2)
    st_dt, st_prev = e.time_dep_state()
    want_dt, want = dt.copy(), n_prev.copy()
    want_dt[1:3], want[1:3] = 2.5, now[1:3]
    assert np.array_equal(st_dt, want_dt) and np.array_equal(st_prev.view(np.uint64), want.view(np.uint64))
    d1, p1 = e.time_dep_state(1, 2)
    assert np.array_equal(d1, want_dt[1:3]) and np.array_equal(p1.view(np.uint64), want[1:3].view(np.uint64))
    assert np.array_equal(e.get(N).view(np.uint64), now.view(np.uint64))           # start does not touch the populations
    e.close()


def ng_history_and_options(lib):
    e, prob, block, a, dt, n_prev = probe_engine(lib, 4, seed=82)
    plain = Engine(prob, block.ncol, lib=lib)
    plain.set_columns(0, block)
    opts, sig = plain.effective_options(), plain.options_signature()
    assert (e.effective_options(), e.options_signature()) == (opts, sig)
    e.configure_ng(2, delay=1)
    for _ in range(3):
        e.formal_sol_gamma()
        e.stat_equil()
    before = e.ng_state().stored.copy()
    assert np.all(before == 2)                   # the delay has run, two vectors are stored
    e.time_dep_start(dt[1:3], col0=1, ncol=2)
    after = e.ng_state().stored
    assert np.array_equal(after[1:3], [-1, -1]) and np.array_equal(after[[0, 3, 4]], before[[0, 3, 4]])
    e.configure_ng(0)
    # Ng off again, a step started and updated: the options and their signature never hear of it
    e.time_dep_start(dt)
    e.formal_sol_gamma()
    e.time_dep_update()
    assert (e.effective_options(), e.options_signature()) == (opts, sig)
    e.close()
    plain.close()


def sharding(lib):
    """a column's bits depend neither on the context's column count nor on the column's index"""
    e, prob, block, a, dt, n_prev = probe_engine(lib, 6, seed=83)
    e.formal_sol_gamma()
    e.time_dep_start(dt, n_prev)
    e.time_dep_update()
    n_all, dP_all = e.get(N), e.get(DP)
    e.close()
    for c in (0, 3, 4):
        one = Engine(prob, 1, lib=lib)
        one.set_columns(0, block.slice(c, c + 1))
        one.formal_sol_gamma()
        one.time_dep_start(dt[c:c + 1], n_prev[c:c + 1])
        one.time_dep_update()
        assert np.array_equal(one.get(N)[0].view(np.uint64), n_all[c].view(np.uint64)), c
        assert one.get(DP)[0] == dP_all[c]
        one.close()


# ---- the driver -------------------------------------------------------------------------------------------------------------
def driver_closed_form(lib):
    """two levels, constant rates, three columns with different dt, five steps: after step m the deviation from equilibrium is
    (1 + dt (C_01 + C_10))^-m times the initial one, within m x the per-step bar"""
    Ns, nc, nsteps = 7, 3, 5
    prob, block, (a,) = probe_problem([2], Ns, nc)
    rng = np.random.default_rng(12)
    Cs = np.zeros((nc, 2, 2, Ns))
    Cs[:, 0, 1] = 10.0 ** rng.uniform(-1, 1, (nc, Ns))          # 1 -> 0
    Cs[:, 1, 0] = 10.0 ** rng.uniform(-1, 1, (nc, Ns))          # 0 -> 1
    n = 1e14 * 10.0 ** rng.uniform(-2, 0, (nc, 2, Ns))
    put(prob, block, a, Cs, n, n.sum(1))
    dt = np.array([0.03, 0.4, 7.0])
    o, o2 = prob.lev_off[a], prob.lev2_off[a]
    w = Worst('%s driver closed form' % lib.backend)
    e = Engine(prob, nc, lib=lib)
    e.set_columns(0, block)
    hist = [e.get(N)[:, o:o + 2]]
    counts = []
    for m in range(nsteps):
        counts.append(drivers.advance_time_columns(e, dt, nsteps=1))
        hist.append(e.get(N)[:, o:o + 2])
    G = e.get(G_)[:, o2:o2 + 4].reshape(nc, 2, 2, Ns)
    assert np.array_equal(G[:, 0, 1], Cs[:, 0, 1]) and np.array_equal(G[:, 1, 0], Cs[:, 1, 0])
    counts = np.concatenate(counts)
    assert counts.shape == (nsteps, nc) and np.all(counts >= 1) and np.all(counts < 200)
    e.close()
    worst = 0.0
    for c in range(nc):
        for k in range(Ns):
            C01, C10 = MP.mpf(float(Cs[c, 0, 1, k])), MP.mpf(float(Cs[c, 1, 0, k]))
            damp = 1 / (1 + MP.mpf(float(dt[c])) * (C01 + C10))
            Nt0 = MP.mpf(float(hist[0][c, 0, k])) + MP.mpf(float(hist[0][c, 1, k]))
            eq1 = Nt0 * C10 / (C01 + C10)
            dev0 = MP.mpf(float(hist[0][c, 1, k])) - eq1
            tol = 0.0
            for m in range(1, nsteps + 1):
                prev, new = hist[m - 1][c, :, k], hist[m][c, :, k]
                # the step's own bar, from the exact solve of the step as the library took it (Gamma is constant, so the iterate
                # the last inner iteration started from is the answer itself within the bar, and has its maximum where that has).
                # The per-step bar is the sum of the two components' bars: (I - dt Gamma)^-1 and its powers are column-stochastic,
                # so an error made in one step is carried through the later ones without growing in the 1-norm; the roundings of
                # the float sums b[iE] (u N a step) are far inside, the bars being no smaller than 12 u N.
                x, bar = exact_step(np.ascontiguousarray(G[c, :, :, k]), np.ascontiguousarray(prev), np.ascontiguousarray(new), dt[c])
                tol += float(np.sum(bar))
                want = eq1 + dev0 * damp ** m
                got = float(abs(MP.mpf(float(new[1])) - want))
                worst = max(worst, got / tol)
                assert got <= tol, (c, k, m, got, tol)
                if m == 1:
                    assert abs(float(dev0 * damp)) > 1e3 * tol       # (the deviation being followed is far above the bar)
    print('%s: worst deviation / (m x per-step bar): %.3g' % (w.tag, worst))


def _converged(lib, prob, block, tol=1e-9, max_iter=2000):
    e = Engine(prob, block.ncol, lib=lib)
    e.set_columns(0, block)
    it = drivers.iterate_mali_columns(e, dJ_tol=tol, dPops_tol=tol, max_iter=max_iter)
    assert np.all(it < max_iter)
    return e


def driver_with_radiation(lib, which):
    """MALI to dPops <= 1e-9; then ONE time step with dt x min(rate) >= 1e12 from LTE to the same tolerance reaches the same
    populations within 1e-6 relative; from the converged state a step of 1e-3, 1 or 1e3 s changes nothing by more than 1e-6"""
    if which == 'toy':
        prob, block = spec_problem([ORDINARY], seed=1, Nspace=13, Nrays=3, Nspect=40, ncol=3, phi_compact=True)
    else:
        prob, block, _ = fixtures.load_problem_npz(golden('falc_ca.npz'))
    tol, max_iter = 1e-9, 2000
    e = _converged(lib, prob, block, tol, max_iter)
    n_se = e.get(N)
    G = e.get(G_)
    e.close()
    rate = np.abs(G[G != 0.0]).min()
    dt_long = max(1e30, 1e13 / rate)
    assert dt_long * rate >= 1e12 and np.isfinite(dt_long)
    t = Engine(prob, block.ncol, lib=lib)
    t.set_columns(0, block)
    t.set(N, np.ascontiguousarray(block.nStar))                       # from LTE
    assert prob.Natoms == 1 and np.allclose(block.nStar.sum(1), block.nTotal[:, 0], rtol=1e-12)     # the step conserves sum n_prev
    counts = drivers.advance_time_columns(t, dt_long, nsteps=1, dJ_tol=tol, dPops_tol=tol, max_iter=max_iter)
    assert counts.shape == (1, block.ncol) and np.all(counts < max_iter)
    n_td = t.get(N)
    worst = float(np.max(np.abs(n_td / n_se - 1.0)))
    print('%s %s: time step of %g s from LTE against MALI: %.3g relative, %s inner iterations' % (lib.backend, which, dt_long, worst, counts[0]))
    assert worst <= 1e-6
    for dtv in (1e-3, 1.0, 1e3):
        before = t.get(N)
        counts = drivers.advance_time_columns(t, dtv, nsteps=1, dJ_tol=tol, dPops_tol=tol, max_iter=max_iter)
        assert np.all(counts < max_iter)
        move = float(np.max(np.abs(t.get(N) / before - 1.0)))
        print('%s %s: a step of %g s from the converged state moves the populations by %.3g' % (lib.backend, which, dtv, move))
        assert move <= 1e-6
    t.close()


def context_time_dep_update(lib, lookahead):
    """Context.time_dep_update on the FALC CaII objects: the arrays still alias eqPops, prevTimePops is what the populations were,
    three inner iterations give the Engine-level sequence bit for bit (the Engine of a second Context on the same objects, so that
    both engines were set up by the same calls)"""
    from helpers import build_fakes
    from lightspinner_amd.rh_method import Context
    d = dict(np.load(golden('falc_ca.npz')))
    atmos, spect, eq, bg = build_fakes(d)
    ctx = Context(atmos, spect, eq, bg, lib=lib, lookahead=lookahead)
    twin = Context(*build_fakes(d), lib=lib, lookahead=False)
    e = twin._engine
    dt = 0.5
    start = [np.array(a.n) for a in ctx.activeAtoms]
    assert np.array_equal(np.concatenate(start), e.get(N)[0])
    e.time_dep_start(dt)
    prev = None
    for it in range(3):
        dJ = ctx.formal_sol_gamma_matrices()
        assert dJ == e.formal_sol_gamma()
        dP, prev2 = ctx.time_dep_update(dt, prev)
        if it == 0:
            assert all(np.array_equal(p, s) for p, s in zip(prev2, start))
            assert all(p is not a.n for p, a in zip(prev2, ctx.activeAtoms))
        else:
            assert prev2 is prev
        prev = prev2
        assert dP == e.time_dep_update()
        assert ctx._spec == bool(lookahead)
        n = e.get(N)[0]
        off = 0
        for a in ctx.activeAtoms:
            diff = float(np.max(np.abs(a.n / n[off:off + a.Nlevel] - 1.0)))
            assert np.array_equal(np.asarray(a.n).view(np.uint64), n[off:off + a.Nlevel].view(np.uint64)), (it, diff)
            off += a.Nlevel
    assert ctx.activeAtoms[0].n is eq['CA'].pops
    st_dt, st_prev = ctx._engine.time_dep_state()
    assert st_dt[0] == dt and np.array_equal(st_prev[0], np.concatenate(start))
    assert dP > 0.0 and not np.array_equal(np.concatenate(start), e.get(N)[0])
    ctx.close()
    twin.close()
