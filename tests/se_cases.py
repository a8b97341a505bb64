"""Bodies of the statistical-equilibrium tests (lsx_stat_equil: rh_method.py:710-745), shared by the CPU run on the oracle
(tests/test_stat_equil_systems.py, -m "not gpu") and the GPU run on the HIP library (the same file, -m gpu).

Gamma cannot be set through the ABI, but it can be steered: a "probe" atom has bound-free transitions only, with alpha all zero.
The formal solution then adds exact zeros to it, and the off-diagonals of LSX_GAMMA are the collisional rates C the test chose,
bit for bit (`gamma_is_the_rates` checks that, and the diagonal).  One ordinary atom beside the probes keeps the plan ordinary.

Every system -- the ordinary atom's too -- is checked against an exact solve: A is LSX_GAMMA as the library reads it back, with
row iE = argmax(n) (first maximum) replaced by ones, b = nTotal e_iE, solved by mpmath at 50 digits.  Each population has the bar

    bar_i = 2 * 3 Nl u (|A^-1| P |L| |U| |x|)_i,          u = 2^-53,

the componentwise forward bound of Gaussian elimination with any pivoting (Higham, Accuracy and Stability of Numerical
Algorithms, Thm 9.4: (A + dA) x^ = b with |dA| <= gamma_3n P^T |L^| |U^|, P A = L U; scipy.linalg.lu returns A = p l u, so its p
is that P^T).  L and U are scipy's; the factor 2 covers the computed factors of another pivot sequence standing in for them.
The bar comes from the read-back matrix and the exact solve only.  A bar wider than 1e-5 |x_i| would make the check vacuous:
asserted.

LSX_DPOPS_COL[c] is checked against max |1 - n_old / x| over the column's systems within
max_i (|n_old / x|_i bar_i / |x_i| + 4 u (1 + |n_old / x|_i)): the quotient inherits x's relative bar, and the quotient, the
difference and the two conversions round once each."""
import math

import mpmath
import numpy as np
import pytest
import scipy.linalg

from lightspinner_amd import _capi
from lightspinner_amd.problem import Engine
from toy import spec_problem

U = 2.0 ** -53
NLS = (2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16)
# Nspace x columns: 21 threads (a partial wavefront); 65 threads (a second block that holds one thread)
SHAPES = ((7, 3), (13, 5))
ORDINARY = (3, [('l', 0, 1, .3, .7), ('c', 0, 2, 0, .4)])
MP = mpmath.mp.clone()
MP.dps = 50


# ---- problems ---------------------------------------------------------------------------------------------------------------
def probe_problem(nls, Nspace, ncol, seed=1, ordinary_at=0):
    """the ordinary atom and probe atoms of nls levels (the ordinary one at position `ordinary_at` of the atom list)
    -> (prob, block, [atom index of each probe])"""
    atoms = [(nl, [('c', 0, nl - 1, 0.1, 0.6)]) for nl in nls]
    atoms.insert(ordinary_at, ORDINARY)
    prob, block = spec_problem(atoms, seed=seed, Nspace=Nspace, Nrays=3, Nspect=40, ncol=ncol, phi_compact=True)
    probes = [a for a in range(len(atoms)) if a != ordinary_at]
    for t in prob.trans:
        if t.atom in probes:
            assert not t.is_line
            t.alpha = np.zeros_like(t.alpha)
    return prob, block, probes


def put(prob, block, a, C=None, n=None, nTotal=None):
    """overwrite atom a's rates C [ncol][Nl][Nl][Ns] (C[to][from]), populations n [ncol][Nl][Ns], nTotal [ncol][Ns]"""
    Nl, o, o2 = prob.Nlevel[a], prob.lev_off[a], prob.lev2_off[a]
    if C is not None:
        block.C[:, o2:o2 + Nl * Nl] = np.asarray(C).reshape(block.ncol, Nl * Nl, prob.Nspace)
    if n is not None:
        block.n[:, o:o + Nl] = n
    if nTotal is not None:
        block.nTotal[:, a] = nTotal


def rates_of(prob, C, a):
    Nl, o2 = prob.Nlevel[a], prob.lev2_off[a]
    return C[:, o2:o2 + Nl * Nl].reshape(C.shape[0], Nl, Nl, prob.Nspace)


def start_populations(rng, Nl, nTot, iE, tie=False):
    """populations that sum to nTot with their (first) maximum at level iE; tie: a second, equal maximum behind it"""
    f = 10.0 ** rng.uniform(-3.0, 0.0, Nl)
    f[iE] = 2.0
    if tie and iE < Nl - 1:
        f[rng.integers(iE + 1, Nl)] = 2.0
    n = f * (nTot / f.sum())
    assert int(np.argmax(n)) == iE
    return n


def _ie_of(q, Nl):
    return (0, Nl // 2, Nl - 1)[(q // 3) % 3]


def rate_scale(rng, Nl, q):
    """rates around 1e-6, 1 and 1e6 s^-1 with +-1.5 decades of scatter: the row of ones is the pivot at step 0, somewhere in the
    middle, or never"""
    C = (1e-6, 1.0, 1e6)[q % 3] * 10.0 ** rng.uniform(-1.5, 1.5, (Nl, Nl))
    return C, _ie_of(q, Nl), False


def _relative_bar_in_float64(C, iE):
    """the largest bar_i / |x_i| of the system the rates C make, estimated in float64 from the inputs alone"""
    Nl = C.shape[0]
    A = np.array(C)
    A[np.arange(Nl), np.arange(Nl)] = 0.0
    A[np.arange(Nl), np.arange(Nl)] = -A.sum(0)
    A[iE, :] = 1.0
    inv = np.linalg.inv(A)
    p, l, u = scipy.linalg.lu(A)
    x = np.abs(inv[:, iE])
    return float(np.max(2.0 * 3.0 * Nl * U * (np.abs(inv) @ (p @ (np.abs(l) @ np.abs(u))) @ x) / x))


def wide_range(rng, Nl, q):
    """rates log-uniform over 1e-8 ... 1e8.  A draw whose smallest population would be known to fewer than five digits (a
    relative bar above 2e-6, a fifth of what check_solve accepts as a meaningful bar) is drawn again: one draw in fifty at three to seven levels"""
    iE = _ie_of(q + q // 9, Nl)
    while True:
        C = 10.0 ** rng.uniform(-8.0, 8.0, (Nl, Nl))
        if _relative_bar_in_float64(C, iE) <= 2e-6:
            return C, iE, False


def ties(rng, Nl, q):
    """rates that are small powers of two on a ring j -> j + 1 (every level reachable: a regular system), so that |Gamma_jj|
    equals another entry of its column (one rate out of level j) or 1.0, the row of ones' entry (rates 1/2 + 1/4 + 1/4, 1/2 + 1/2
    or 1); two equal largest populations in two systems of three"""
    C = np.zeros((Nl, Nl))
    for j in range(Nl):
        nxt = (j + 1) % Nl
        others = [i for i in range(Nl) if i not in (j, nxt)]
        kind = rng.integers(0, 3)
        if kind == 0 or not others:
            C[nxt, j] = 1.0 if kind == 1 else 2.0 ** rng.integers(-2, 3)
        elif kind == 1 or len(others) < 2:
            C[nxt, j] = C[rng.choice(others), j] = 0.5
        else:
            a, b = rng.choice(others, 2, replace=False)
            C[nxt, j], C[a, j], C[b, j] = 0.5, 0.25, 0.25
    return C, _ie_of(q, Nl), q % 3 != 2


FAMILIES = dict(rate_scale=rate_scale, wide_range=wide_range, ties=ties)


def family_inputs(family, prob, block, a, seed, ntot_factor=0.3):
    """fill probe atom a of (prob, block) with systems of `family` -> the levels the eliminated row takes"""
    rng = np.random.default_rng(seed)
    Nl, Ns, nc = prob.Nlevel[a], prob.Nspace, block.ncol
    C, n = np.zeros((nc, Nl, Nl, Ns)), np.zeros((nc, Nl, Ns))
    nTot = 1e14 * np.exp(9.0 * np.linspace(0.0, 1.0, Ns))[None, :] * ntot_factor * (1.0 + 0.1 * np.arange(nc))[:, None]
    seen = set()
    for c in range(nc):
        for k in range(Ns):
            Ck, iE, tie = FAMILIES[family](rng, Nl, c * Ns + k)
            Ck[np.arange(Nl), np.arange(Nl)] = 0.0
            C[c, :, :, k] = Ck
            n[c, :, k] = start_populations(rng, Nl, nTot[c, k], iE, tie)
            seen.add(iE)
    put(prob, block, a, C, n, nTot)
    return seen


# ---- the exact reference and its bars ---------------------------------------------------------------------------------------
_exact_cache = {}


def exact_system(G, n_old, nTot):
    """one system: G [Nl][Nl] read back from the library, n_old [Nl] -> (x as mpmath numbers, bar [Nl], pivot rows).  Kept per
    input: the oracle's run and the host build's solve the same systems"""
    key = (np.ascontiguousarray(G).tobytes(), np.ascontiguousarray(n_old).tobytes(), float(nTot))
    if key not in _exact_cache:
        _exact_cache[key] = _exact_system(G, n_old, nTot)
    return _exact_cache[key]


def _exact_system(G, n_old, nTot):
    Nl = G.shape[0]
    iE = int(np.argmax(n_old))
    A = np.array(G, dtype=np.float64)
    A[iE, :] = 1.0
    Ainv = MP.inverse(MP.matrix(A.tolist()))
    x = [Ainv[i, iE] * MP.mpf(float(nTot)) for i in range(Nl)]
    absinv = np.array([[float(abs(Ainv[i, j])) for j in range(Nl)] for i in range(Nl)])
    p, l, u = scipy.linalg.lu(A)
    absx = np.array([float(abs(v)) for v in x])
    bar = 2.0 * 3.0 * Nl * U * (absinv @ (p @ (np.abs(l) @ np.abs(u))) @ absx)
    return x, bar, tuple(int(r) for r in np.argmax(p, axis=0))


class Worst:
    """largest measured-to-bar ratios, per number of levels (printed by the tests; asserted <= 1 entry by entry)"""
    def __init__(self, tag):
        self.tag, self.pops, self.mon, self.relbar = tag, {}, 0.0, 0.0

    def report(self):
        print('%s: deviation / bar of the populations: %s; of DPOPS_COL: %.3g; largest relative bar: %.3g' % (
            self.tag, ', '.join('Nl %d: %.3g' % kv for kv in sorted(self.pops.items())), self.mon, self.relbar))


def check_solve(w, prob, G, n_old, n_new, nTotal, dPcol, singular=(), active=None):
    """checks 1 and 3: every system of every atom of every active column against the exact solve, and LSX_DPOPS_COL.
    singular: {(col, atom, depth)} made singular on purpose -- populations bit-identical to before, nothing for the monitor.
    -> {atom: pivot permutations scipy's LU takes on its systems}"""
    ncol, Ns = G.shape[0], prob.Nspace
    perms = {a: set() for a in range(prob.Natoms)}
    for c in range(ncol):
        if active is not None and not active[c]:
            assert np.array_equal(n_new[c], n_old[c], equal_nan=True), 'frozen column %d: populations changed' % c
            assert dPcol[c] == 0.0
            continue
        ch_max, ch_bar = 0.0, 0.0
        for a in range(prob.Natoms):
            Nl, o, o2 = prob.Nlevel[a], prob.lev_off[a], prob.lev2_off[a]
            Ga = G[c, o2:o2 + Nl * Nl].reshape(Nl, Nl, Ns)
            for k in range(Ns):
                old, new = n_old[c, o:o + Nl, k], n_new[c, o:o + Nl, k]
                if (c, a, k) in singular:
                    assert np.array_equal(old.view(np.uint64), new.view(np.uint64)), 'singular system %r: populations changed' % ((c, a, k),)
                    continue
                x, bar, perm = exact_system(Ga[:, :, k], old, nTotal[c, a, k])
                perms[a].add(perm)
                for i in range(Nl):
                    ax = float(abs(x[i]))
                    assert ax > 0.0 and bar[i] <= 1e-5 * ax, 'vacuous bar %.3g at %r' % (bar[i] / ax, (c, a, k, i))
                    w.relbar = max(w.relbar, bar[i] / ax)
                    dev = float(abs(MP.mpf(float(new[i])) - x[i]))
                    r = dev / bar[i]
                    w.pops[Nl] = max(w.pops.get(Nl, 0.0), r)
                    assert r <= 1.0, '%s: population at column %d, atom %d, depth %d, level %d: %.3g x the bar (%r, exact %s)' % (
                        w.tag, c, a, k, i, r, new[i], MP.nstr(x[i], 20))
                    q = float(abs(MP.mpf(float(old[i])) / x[i]))
                    ch_max = max(ch_max, float(abs(1 - MP.mpf(float(old[i])) / x[i])))
                    ch_bar = max(ch_bar, q * bar[i] / ax + 4.0 * U * (1.0 + q))
        r = abs(dPcol[c] - ch_max) / ch_bar
        w.mon = max(w.mon, r)
        assert r <= 1.0, '%s: DPOPS_COL[%d] = %r, exact %r: %.3g x the bar' % (w.tag, c, dPcol[c], ch_max, r)
    return perms


def run(lib, prob, block, options=None, calls='sync'):
    """FS; SE on a fresh engine -> (engine, Gamma, n before, n after, DPOPS_COL, dPops)"""
    e = Engine(prob, block.ncol, lib=lib, options=options)
    e.set_columns(0, block)
    e.formal_sol_gamma()
    G, n_old = e.get(_capi.LSX_GAMMA), e.get(_capi.LSX_N)
    dP = solve(e, calls)
    return e, G, n_old, e.get(_capi.LSX_N), e.get(_capi.LSX_DPOPS_COL), dP


def solve(e, calls):
    """one statistical equilibrium: blocking, or enqueued with the next formal solution behind it and one read at the end"""
    if calls == 'sync':
        return e.stat_equil()
    e.stat_equil_async()
    e.formal_sol_gamma_async()
    return e.sync()[1]


# ---- 1-3: the families ----------------------------------------------------------------------------------------------------------
def family(lib, name, Nl, results=None, check=True):
    """one family at one size on both context shapes.  results: dict that receives the new populations (for hip vs oracle;
    check=False: nothing else is wanted)"""
    w = Worst('%s %s Nl=%d' % (lib.backend, name, Nl))
    perms, seen = set(), set()
    for s, (Ns, nc) in enumerate(SHAPES):
        prob, block, (a,) = probe_problem([Nl], Ns, nc)
        seen |= family_inputs(name, prob, block, a, seed=1000 * Nl + s)
        e, G, n_old, n_new, dPcol, dP = run(lib, prob, block)
        e.close()
        if results is not None:
            results[(name, Nl, s)] = (n_new, G)
        if not check:
            continue
        perms |= check_solve(w, prob, G, n_old, n_new, block.nTotal, dPcol)[a]
        assert dP == dPcol.max()
    if not check:
        return None
    assert seen == {0, Nl // 2, Nl - 1}
    if name == 'rate_scale':
        # the eliminated row's 1.0 wins the pivot search at step 0, later, or not before the last step: at two levels that makes
        # both row orders, at three all four that scipy's LU can reach with one row of ones, from there on at least four
        want = {2: 2, 3: 4}.get(Nl, 4)
        assert len(perms) >= want, 'Nl=%d: %d distinct pivot sequences' % (Nl, len(perms))
    w.report()
    return w


def two_probe_atoms(lib, results=None):
    """probes of 4 and 9 levels (a register instance and the LDS kernel) behind the ordinary atom, different nTotal: the level
    offsets of the second and third atom, and the per-atom launches"""
    w = Worst('%s two probes' % lib.backend)
    for s, (Ns, nc) in enumerate(SHAPES):
        prob, block, (a, b) = probe_problem([4, 9], Ns, nc)
        family_inputs('rate_scale', prob, block, a, seed=77 + s, ntot_factor=0.3)
        family_inputs('wide_range', prob, block, b, seed=78 + s, ntot_factor=0.011)
        e, G, n_old, n_new, dPcol, dP = run(lib, prob, block)
        check_solve(w, prob, G, n_old, n_new, block.nTotal, dPcol)
        if results is not None:
            results[('two', 0, s)] = (n_new, G)
        e.close()
    w.report()
    return w


# ---- 4: Gamma of a probe atom is its rates ---------------------------------------------------------------------------------
def gamma_is_the_rates(lib, options=None):
    """every off-diagonal of a probe atom's Gamma is its C bit for bit; Gamma_jj = -sum_{i != j} C_ij within the (Nl - 1)
    roundings of a sum of Nl - 1 positive terms"""
    for Nl in (2, 5, 9, 16):
        Ns, nc = SHAPES[0]
        prob, block, (a,) = probe_problem([Nl], Ns, nc)
        family_inputs('wide_range', prob, block, a, seed=40 + Nl)
        e = Engine(prob, nc, lib=lib, options=options)
        e.set_columns(0, block)
        e.formal_sol_gamma()
        G, C = rates_of(prob, e.get(_capi.LSX_GAMMA), a), rates_of(prob, block.C, a)
        e.close()
        for c in range(nc):
            for k in range(Ns):
                for j in range(Nl):
                    col = [float(C[c, i, j, k]) for i in range(Nl) if i != j]
                    for i in range(Nl):
                        if i != j:
                            assert G[c, i, j, k].view(np.uint64) == C[c, i, j, k].view(np.uint64), (Nl, c, i, j, k)
                    want = -math.fsum(col)
                    assert abs(G[c, j, j, k] - want) <= (Nl - 1) * U * math.fsum(col), (Nl, c, j, k, G[c, j, j, k], want)


# ---- 5: one singular system among regular ones ------------------------------------------------------------------------------
def expect_singular(e, calls, col, depth, atom):
    with pytest.raises(_capi.LsxSingularError, match=r'column %d, depth %d, atom %d\b' % (col, depth, atom)) as ei:
        solve(e, calls)
    assert ei.value.code == _capi.LSX_ESINGULAR


def one_singular_system(lib, calls, Nl=5):
    """C of the probe atom zeroed at one (column, depth): LSX_ESINGULAR names that system, its populations keep their bits, every
    other system is solved and monitored as usual; frozen, the column raises nothing; repaired, the same context goes on"""
    Ns, nc = SHAPES[1]
    sc, sk = 3, 12                      # thread 51 of block 0; the column also holds the one thread of block 1 (column 4, depth 12: no)
    prob, block, (a,) = probe_problem([Nl], Ns, nc)
    family_inputs('rate_scale', prob, block, a, seed=5)
    good = rates_of(prob, block.C, a).copy()
    bad = good.copy()
    bad[sc, :, :, sk] = 0.0
    put(prob, block, a, C=bad)
    w = Worst('%s one singular (%s)' % (lib.backend, calls))
    e = Engine(prob, nc, lib=lib)
    e.set_columns(0, block)
    e.formal_sol_gamma()
    G, n_old = e.get(_capi.LSX_GAMMA), e.get(_capi.LSX_N)
    expect_singular(e, calls, sc, sk, a)
    n_new, dPcol = e.get(_capi.LSX_N), e.get(_capi.LSX_DPOPS_COL)
    check_solve(w, prob, G, n_old, n_new, block.nTotal, dPcol, singular={(sc, a, sk)})
    # the column that holds it frozen: nothing raised, nothing changed there, DPOPS_COL 0
    e.set_columns(0, block)
    e.formal_sol_gamma()
    active = np.ones(nc, dtype=bool)
    active[sc] = False
    e.set_active_columns(active)
    e.formal_sol_gamma()
    G = e.get(_capi.LSX_GAMMA)
    solve(e, calls)
    check_solve(w, prob, G, n_old, e.get(_capi.LSX_N), block.nTotal, e.get(_capi.LSX_DPOPS_COL), active=active)
    e.set_active_columns(None)
    # repaired: FS; SE on the same context
    put(prob, block, a, C=good)
    e.set_columns(0, block)
    e.formal_sol_gamma()
    G = e.get(_capi.LSX_GAMMA)
    solve(e, calls)
    check_solve(w, prob, G, n_old, e.get(_capi.LSX_N), block.nTotal, e.get(_capi.LSX_DPOPS_COL))
    e.close()
    w.report()
    return w


# ---- 6: which singular system is "the first" ------------------------------------------------------------------------------------
def first_singular_system(lib):
    """column 1 singular at (atom 1, depth 2) and at (atom 0, depth 5), column 2 at (atom 0, depth 0): the reference walks atoms
    outside depths (rh_method.py:720-739) and columns one after the other (response_fn.py:61-65), so what it raises on first is
    the lowest column, then the lowest atom, then the lowest depth: column 1, atom 0, depth 5"""
    Ns, nc = SHAPES[0]
    prob, block, (a, b) = probe_problem([4, 5], Ns, nc, ordinary_at=2)
    assert (a, b) == (0, 1)
    family_inputs('rate_scale', prob, block, a, seed=61)
    family_inputs('rate_scale', prob, block, b, seed=62)
    Ca, Cb = rates_of(prob, block.C, a).copy(), rates_of(prob, block.C, b).copy()
    Cb[1, :, :, 2] = 0.0
    Ca[1, :, :, 5] = 0.0
    Ca[2, :, :, 0] = 0.0
    put(prob, block, a, C=Ca)
    put(prob, block, b, C=Cb)
    w = Worst('%s first singular' % lib.backend)
    for calls in ('sync', 'async'):
        e = Engine(prob, nc, lib=lib)
        e.set_columns(0, block)
        e.formal_sol_gamma()
        G, n_old = e.get(_capi.LSX_GAMMA), e.get(_capi.LSX_N)
        expect_singular(e, calls, 1, 5, 0)
        check_solve(w, prob, G, n_old, e.get(_capi.LSX_N), block.nTotal, e.get(_capi.LSX_DPOPS_COL),
                    singular={(1, 1, 2), (1, 0, 5), (2, 0, 0)})
        e.close()


# ---- 7: NaN -----------------------------------------------------------------------------------------------------------------
def nan_in_the_rates(lib, Nl):
    """one NaN in C of the probe atom, at one system per position: in the eliminated row (only the NaN it leaves on the diagonal
    of its column remains), below the diagonal, above it, in the last column, in the last row.  The reference aborts before it
    writes anything (scipy.linalg.solve, check_finite); the libraries report LSX_ESINGULAR for that system, leave its populations
    alone and solve the others"""
    Ns, nc = SHAPES[1]
    w = Worst('%s NaN Nl=%d' % (lib.backend, Nl))
    prob, block, (a,) = probe_problem([Nl], Ns, nc)
    family_inputs('rate_scale', prob, block, a, seed=7)
    n = block.n[:, prob.lev_off[a]:prob.lev_off[a] + Nl]
    good = rates_of(prob, block.C, a).copy()
    sc, sk = 2, 9
    iE = int(np.argmax(n[sc, :, sk]))
    spots = {(iE, (iE + 1) % Nl), (Nl - 1, 0), (0, Nl - 1), (Nl - 2, Nl - 1), (Nl - 1, Nl - 2), (Nl // 2, max(0, Nl // 2 - 1))}
    for i, j in sorted(s for s in spots if s[0] != s[1]):
        bad = good.copy()
        bad[sc, i, j, sk] = np.nan
        put(prob, block, a, C=bad)
        e = Engine(prob, nc, lib=lib)
        e.set_columns(0, block)
        e.formal_sol_gamma()
        G, n_old = e.get(_capi.LSX_GAMMA), e.get(_capi.LSX_N)
        assert np.isnan(rates_of(prob, G, a)[sc, j, j, sk])
        expect_singular(e, 'sync', sc, sk, a)
        check_solve(w, prob, G, n_old, e.get(_capi.LSX_N), block.nTotal, e.get(_capi.LSX_DPOPS_COL), singular={(sc, a, sk)})
        e.close()
    return w


# ---- the host build of the device's solve (td_cases.HostLib) on the oracle's Gamma -------------------------------------------
def oracle_gamma(oracle_lib, prob, block):
    e = Engine(prob, block.ncol, lib=oracle_lib)
    e.set_columns(0, block)
    e.formal_sol_gamma()
    G, n_old = e.get(_capi.LSX_GAMMA), e.get(_capi.LSX_N)
    e.close()
    return G, n_old


def host_forms(host, prob, G, nTotal, n_old, Nl, singular=frozenset()):
    """the form the device runs for this size; up to 8 levels, the in-memory form at work strides 1 and 64 gives its bits"""
    n_new, dPcol, flagged = host.solve(prob, G, nTotal, n_old)
    assert flagged == set(singular)
    for stride in (1, 64) if Nl <= 8 else ():
        n_mem, dP_mem, fl_mem = host.solve(prob, G, nTotal, n_old, in_memory=True, work_stride=stride)
        assert np.array_equal(n_mem.view(np.uint64), n_new.view(np.uint64)), (Nl, stride)
        assert np.array_equal(dP_mem.view(np.uint64), dPcol.view(np.uint64)), (Nl, stride)
        assert fl_mem == flagged
    return n_new, dPcol


def host_family(oracle_lib, host, name, Nl):
    """`family` with Gamma and n from the oracle's formal solution and the solve from the host build: the same inputs, the same
    checker, the same bars"""
    w = Worst('host %s Nl=%d' % (name, Nl))
    for s, (Ns, nc) in enumerate(SHAPES):
        prob, block, (a,) = probe_problem([Nl], Ns, nc)
        family_inputs(name, prob, block, a, seed=1000 * Nl + s)
        G, n_old = oracle_gamma(oracle_lib, prob, block)
        n_new, dPcol = host_forms(host, prob, G, block.nTotal, n_old, Nl)
        check_solve(w, prob, G, n_old, n_new, block.nTotal, dPcol)
    w.report()
    return w


def host_bad_systems(oracle_lib, host, Nl):
    """one singular system (its rates zeroed, as one_singular_system) and one with a NaN rate (as nan_in_the_rates) among regular
    ones: both flagged and nothing else, their populations bit-identical to before, the others solved and monitored as usual"""
    Ns, nc = SHAPES[1]
    prob, block, (a,) = probe_problem([Nl], Ns, nc)
    family_inputs('rate_scale', prob, block, a, seed=5)
    bad = rates_of(prob, block.C, a).copy()
    bad[3, :, :, 12] = 0.0
    bad[2, Nl - 1, 0, 9] = np.nan
    put(prob, block, a, C=bad)
    G, n_old = oracle_gamma(oracle_lib, prob, block)
    singular = {(3, a, 12), (2, a, 9)}
    n_new, dPcol = host_forms(host, prob, G, block.nTotal, n_old, Nl, singular)
    w = Worst('host bad systems Nl=%d' % Nl)
    check_solve(w, prob, G, n_old, n_new, block.nTotal, dPcol, singular=singular)
    w.report()


# ---- 8, 9: HIP only ---------------------------------------------------------------------------------------------------------
def too_many_levels(lib):
    """atoms of 3 and 17 levels: 17 x 17 + 2 x 17 doubles for each of 64 threads exceed the 160 KiB of LDS (16 levels fit: the
    families run them).  lsx_create refuses the problem with LSX_EUNSUPPORTED, so no statistical equilibrium can fail partway"""
    Ns, nc = SHAPES[0]
    prob, block, (a,) = probe_problem([17], Ns, nc)
    assert prob.Nlevel == [3, 17]
    for options in (None, 'se_lds=1'):
        with pytest.raises(_capi.LsxError, match='Nlevel = 17 needs 165376 B') as ei:
            Engine(prob, nc, lib=lib, options=options)
        assert ei.value.code == _capi.LSX_EUNSUPPORTED


def instances_agree(lib, Nl):
    """se_lds=1 (the LDS kernel for every size) gives the bits of the register instance"""
    for name in FAMILIES:
        Ns, nc = SHAPES[1]
        prob, block, (a,) = probe_problem([Nl], Ns, nc)
        family_inputs(name, prob, block, a, seed=90 + Nl)
        out = []
        for options in (None, 'se_lds=1'):
            e, G, n_old, n_new, dPcol, dP = run(lib, prob, block, options=options)
            assert ('se_lds=1' in e.effective_options()) == (options is not None)
            out.append((n_new, dPcol))
            e.close()
        assert np.array_equal(out[0][0].view(np.uint64), out[1][0].view(np.uint64)), (name, Nl)
        assert np.array_equal(out[0][1].view(np.uint64), out[1][1].view(np.uint64)), (name, Nl)
        assert not np.array_equal(out[0][0], n_old)


def hip_against_oracle(rh, ro):
    """reported, not asserted: the largest |hip - oracle| of the new populations in units of u |x|, and whether the two libraries
    solved the same matrices (their Gamma diagonals are sums in different orders)"""
    worst, same = 0.0, True
    for key in rh:
        worst = max(worst, float((np.abs(rh[key][0] - ro[key][0]) / (U * np.abs(ro[key][0]))).max()))
        same = same and np.array_equal(rh[key][1], ro[key][1])
    name, Nl = next(iter(rh))[:2]
    print('hip vs oracle, %s Nl=%d: largest |difference| / (u |x|): %.3g (Gamma %s)' % (name, Nl, worst, 'identical' if same else 'differs'))
    return worst
