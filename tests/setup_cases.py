"""Bodies of the set-up chain tests (lsx_set_atomic_data / lsx_set_atmosphere / lsx_set_line_profiles), shared by the CPU run
on the oracle (tests/test_setup_atoms.py, -m "not gpu") and the GPU run on the HIP library (the same file, -m gpu).

Every comparison is entry by entry, relative to the entry itself, inside a bar derived from the operations that produce it
(EPS = 2^-52 is one ulp at 1; each bar counts the roundings on the library's path AND on the reference's):
  * vBroad = sqrt(vTherm T + vturb^2): 4 roundings each side.
  * aDamp = (gRad + Qelast) cDop / vBroad: a sum of positive terms, each a product of at most 12 roundings and 3 pow() calls
    (<= 2 ulp each) -> 32 EPS.
  * nStar_i = g_i0 exp(-x_i) / cNe_T^dZ n_0 with x_i = dE_i / kT: exp turns the argument's relative rounding (<= 4 EPS each side)
    into an absolute one, |x_i| 8 EPS; n_0 = nTotal / sum_l (...) carries the largest of the sum's terms' errors.
  * a spline value carries 12 roundings of the magnitude of its terms over its value, plus the first-order effect of the
    moments' rounding error (`spline_terms`, `moment_errors`), on each side.
  * a rate entry is a sum of collisions' contributions: each carries its spline bar, 16 EPS of products, |dE / kT| 8 EPS for a CI's
    exp and the two Boltzmann factors of nStar_i / nStar_j; the entry's bar is sum(|contribution| bar) / |entry|.
Entries the reference clamps to zero (C[C < 0] = 0, rh_method.py:487) must be exactly 0."""
import numpy as np
import pytest
from scipy.interpolate import interp1d, make_interp_spline

from conftest import golden
from lightspinner_amd import fixtures, atomdata, _capi, constants as K
from lightspinner_amd.problem import Engine, ColumnBlock

EPS = np.finfo(np.float64).eps
C0_OMEGA = 2.1798741E-18 / np.sqrt(K.MElectron) * np.pi * 5.29177349E-11 ** 2 * np.sqrt(8.0 / (np.pi * K.KBoltzmann))   # collisional_rates.py:38


def _ratio(dev, bar):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(bar > 0, dev / bar, np.where(dev > 0, np.inf, 0.0))


class Ledger:
    """largest measured-to-bar ratio per quantity (printed by the tests, asserted <= 1 entry by entry)"""
    def __init__(self, tag):
        self.tag, self.worst = tag, {}

    def check(self, what, got, ref, bar_rel):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        r = _ratio(np.abs(got - ref), np.asarray(bar_rel) * np.abs(ref))
        worst = float(np.max(r)) if r.size else 0.0
        self.worst[what] = max(self.worst.get(what, 0.0), worst)
        assert worst <= 1.0, '%s %s: %.3g x the bar at %s' % (self.tag, what, worst, np.unravel_index(np.argmax(r), r.shape))

    def report(self):
        print('%s: largest measured / bar: %s' % (self.tag, ', '.join('%s %.3g' % kv for kv in sorted(self.worst.items()))))
        return self.worst


# ---- the reference's formulas in numpy, for the bars and for the reference-free spline test ------------------------------
def moment_errors(x, y, M):
    """first-order bound on the rounding error of the not-a-knot moments M (second derivatives at the knots) in units of EPS:
    the right side 6 (s_i - s_i-1) of the tridiagonal rows is a difference of slopes (4 roundings of |6 s_i| + |6 s_i-1|), the
    matrix entries are differences of knots (2 roundings); |A^-1| (|db| + |dA| |M|)"""
    n = x.shape[0]
    h = np.diff(x)
    A = np.zeros((n, n))
    bm = np.zeros(n)
    A[0, :3] = h[1], -(h[0] + h[1]), h[0]
    A[n - 1, n - 3:] = h[n - 2], -(h[n - 3] + h[n - 2]), h[n - 3]
    s = np.diff(y) / h
    for i in range(1, n - 1):
        A[i, i - 1:i + 2] = h[i - 1], 2.0 * (h[i - 1] + h[i]), h[i]
        bm[i] = 6.0 * (np.abs(s[i]) + np.abs(s[i - 1]))
    return np.abs(np.linalg.inv(A)) @ (4.0 * bm + 2.0 * np.abs(A) @ np.abs(M))


def spline_terms(x, y, t):
    """-> (value, error bound in units of EPS) of the interpolant interp1d(x, y, kind=3 | linear for 2 points,
    fill_value=(y[0], y[-1])) at t, written as the library evaluates it:
    M_i a^3 / 6h + M_i+1 b^3 / 6h + (y_i / h - M_i h / 6) a + (y_i+1 / h - M_i+1 h / 6) b.  The bound: 12 roundings of the
    magnitude of those terms, plus what the moments' own error (moment_errors) does to them"""
    x, y, t = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(t, dtype=np.float64)
    n = x.shape[0]
    M = np.zeros(n) if n == 2 else make_interp_spline(x, y, k=3).derivative(2)(x)
    dM = np.zeros(n) if n == 2 else moment_errors(x, y, M)
    i = np.clip(np.searchsorted(x, t, side='left') - 1, 0, n - 2)
    h, a, b = x[i + 1] - x[i], x[i + 1] - t, t - x[i]
    terms = np.stack([M[i] * a ** 3 / (6 * h), M[i + 1] * b ** 3 / (6 * h), (y[i] / h - M[i] * h / 6) * a, (y[i + 1] / h - M[i + 1] * h / 6) * b])
    kind = 'linear' if n == 2 else 3
    val = interp1d(x, y, kind=kind, fill_value=(y[0], y[-1]), bounds_error=False)(t)
    err = 12.0 * np.abs(terms).sum(0) + dM[i] * np.abs(a ** 3 - a * h * h) / (6 * h) + dM[i + 1] * np.abs(b ** 3 - b * h * h) / (6 * h)
    err = np.where((t < x[0]) | (t > x[-1]), 0.0, err)
    return val, err


def boltzmann_args(E, T):
    """|dE_i / kT| of every level against the ground level: [Nl][Ns]"""
    return np.abs((np.asarray(E)[:, None] - E[0]) / (K.KBoltzmann * np.asarray(T)[None, :]))


def nstar_bar(E, T):
    x = boltzmann_args(E, T)
    return EPS * (16.0 + 8.0 * x + 8.0 * x.max(axis=0, keepdims=True))


def rate_contributions(atom, T, ne, nStar):
    """-> [(to, from, contribution [Ns], relative bar [Ns])] of every collision of `atom` (atomdata.AtomData), the reference's
    formulas (collisional_rates.py:38-45, 62-70, 88-96) in float64 on the given nStar"""
    T, ne = np.asarray(T, dtype=np.float64), np.asarray(ne, dtype=np.float64)
    xb = boltzmann_args(atom.E_SI, T)
    out = []
    for k in atom.collisions:
        i, j = k.i, k.j
        v, err = spline_terms(k.temperature, k.rates, T)
        with np.errstate(divide='ignore', invalid='ignore'):
            sb = 2.0 * EPS * np.where(err > 0, err / np.abs(v), 0.0)          # the library's evaluation and the reference's
        ratio_bar = 8.0 * EPS * (xb[i] + xb[j] + 2.0)
        if k.kind == _capi.LSX_COLL_OMEGA:
            down = C0_OMEGA * ne * v / (atom.g[j] * np.sqrt(T))
            out += [(i, j, down, sb + 16 * EPS), (j, i, down * nStar[j] / nStar[i], sb + 16 * EPS + ratio_bar)]
        elif k.kind == _capi.LSX_COLL_CI:
            x = (atom.E_SI[j] - atom.E_SI[i]) / (K.KBoltzmann * T)
            up = v * ne * np.exp(-x) * np.sqrt(T)
            eb = sb + 16 * EPS + 8 * EPS * x
            out += [(j, i, up, eb), (i, j, up * nStar[i] / nStar[j], eb + ratio_bar)]
        else:
            down = v * ne * (atom.g[i] / atom.g[j]) * np.sqrt(T)
            out += [(i, j, down, sb + 16 * EPS), (j, i, down * nStar[j] / nStar[i], sb + 16 * EPS + ratio_bar)]
    return out


def rates_and_bars(atom, T, ne, nStar):
    """-> (C [Nl][Nl][Ns] with the clamp, absolute bar [Nl][Nl][Ns])"""
    Nl = len(atom.g)
    C = np.zeros((Nl, Nl, len(T)))
    B = np.zeros_like(C)
    for to, fr, c, bar in rate_contributions(atom, T, ne, nStar):
        C[to, fr] += c
        B[to, fr] += np.abs(c) * bar
    C[C < 0.0] = 0.0
    return C, B


def check_rates(led, what, got, ref, bar_abs):
    """per entry: |got - ref| <= bar; entries the reference clamped to 0 are exactly 0"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    zero = ref == 0.0
    assert np.all(got[zero] == 0.0), '%s: %d entries the reference holds at 0 are not 0' % (what, int(np.sum(got[zero] != 0.0)))
    assert np.all(got >= 0.0)
    r = _ratio(np.abs(got - ref), bar_abs)
    worst = float(np.max(r))
    led.worst[what] = max(led.worst.get(what, 0.0), worst)
    assert worst <= 1.0, '%s: %.3g x the bar at %s (got %r, reference %r)' % (
        what, worst, np.unravel_index(np.argmax(r), r.shape), got.flat[np.argmax(r)], ref.flat[np.argmax(r)])


def check_setup_against_reference(led, atoms, prob, T, vB, aD, nStar, n, C, ref, factor=1.0):
    """one column of a library's set-up outputs against the reference's: ref = dict(ne, and per atom vBroad, nStar, C, aDamp
    (rows in the context's line order)).  factor 2: ref is another library that is itself inside the bars"""
    lo = 0
    for a, atom in enumerate(atoms):
        tag = '%s %s' % (led.tag, prob.atom_names[a])
        led.check('vBroad', vB[a], ref['vBroad'][a], factor * 4 * EPS)
        nl = ref['aDamp'][a].shape[0]
        led.check('aDamp', aD[lo:lo + nl], ref['aDamp'][a], factor * 32 * EPS)
        lo += nl
        o, Nl = prob.lev_off[a], prob.Nlevel[a]
        led.check('nStar', nStar[o:o + Nl], ref['nStar'][a], factor * nstar_bar(atom.E_SI, T))
        assert np.array_equal(n[o:o + Nl], nStar[o:o + Nl]), tag          # n starts as a copy of nStar, rh_method.py:414-416
        o2 = prob.lev2_off[a]
        _, B = rates_and_bars(atom, T, ref['ne'], ref['nStar'][a])
        check_rates(led, 'C', C[o2:o2 + Nl * Nl].reshape(Nl, Nl, -1), ref['C'][a], factor * B)
    assert lo == aD.shape[0]


def setup_outputs(e):
    """-> (vBroad, aDamp, nStar, n, C) of an engine"""
    return tuple(e.get(w) for w in (_capi.LSX_VBROAD, _capi.LSX_ADAMP, _capi.LSX_NSTAR, _capi.LSX_N, _capi.LSX_C))


def against_each_other(e1, e2, tag):
    """two libraries' outputs of five_atoms_against_the_reference, each inside the bars around the reference: within twice
    those bars of each other, entry by entry"""
    from lightspinner_amd.fixtures import load_problem_npz
    s = dict(np.load(golden('setup_atoms.npz')))
    prob, _, raw = load_problem_npz(golden('falc_all.npz'))
    data = atomdata.from_fixture(s)
    a1, a2 = setup_outputs(e1), setup_outputs(e2)
    led = Ledger(tag)
    for c, (T, ne) in enumerate(((raw['temperature'], raw['ne']), (s['edge_temperature'], s['edge_ne']))):
        vB, aD, nStar, n, C = (x[c] for x in a2)
        lines, ref = 0, dict(ne=ne, vBroad=vB, nStar=[], C=[], aDamp=[])
        for a in range(prob.Natoms):
            o, o2, Nl = prob.lev_off[a], prob.lev2_off[a], prob.Nlevel[a]
            nl = sum(1 for t in prob.trans if t.atom == a and t.is_line)
            ref['nStar'].append(nStar[o:o + Nl]); ref['C'].append(C[o2:o2 + Nl * Nl].reshape(Nl, Nl, -1))
            ref['aDamp'].append(aD[lines:lines + nl]); lines += nl
        check_setup_against_reference(led, data.atoms, prob, T, *(x[c] for x in a1), ref, factor=2.0)
    led.report()


# ---- test 1: five atoms, FALC and the edge column ----------------------------------------------------------------------
def five_atoms_against_the_reference(lib):
    """the falc_all problem with two columns, FALC and `edge` (tests/golden/setup_atoms.npz: 400 K ... 1e6 K, every table knot,
    ne 1e12 ... 1e23 m^-3): the library's vBroad, aDamp, nStar and C against the reference's, entry by entry -> (engine, ledger)"""
    s = dict(np.load(golden('setup_atoms.npz')))
    prob, block, raw = fixtures.load_problem_npz(golden('falc_all.npz'))
    assert [str(x) for x in raw['atom_names']] == [str(x) for x in s['atom_names']]
    data = atomdata.from_fixture(s)
    e = Engine(prob, 2, lib=lib)
    e.set_columns(0, ColumnBlock.concatenate([block, block]))
    e.set_atomic_data(data)
    Na = prob.Natoms
    e.set_atmosphere(0, lte_pops=True, temperature=np.stack([raw['temperature'], s['edge_temperature']]),
                     ne=np.stack([raw['ne'], s['edge_ne']]), vturb=np.stack([raw['vturb'], s['edge_vturb']]),
                     nHGround=np.stack([raw['hGround'], s['edge_hGround']]),
                     nTotal=np.stack([np.stack([raw['a%d_nTotal' % a] for a in range(Na)]),
                                      np.stack([s['edge_a%d_nTotal' % a] for a in range(Na)])]))
    vB, aD, nStar, n, C = setup_outputs(e)
    lines = [[kr for kr in range(len(prob.trans)) if prob.trans[kr].atom == a and prob.trans[kr].is_line] for a in range(Na)]
    falc = dict(ne=raw['ne'], vBroad=[raw['a%d_vBroad' % a] for a in range(Na)], nStar=[raw['a%d_nStar' % a] for a in range(Na)],
                C=[raw['a%d_C' % a] for a in range(Na)], aDamp=[np.array([raw['t%d_aDamp' % kr] for kr in lines[a]]) for a in range(Na)])
    edge = dict(ne=s['edge_ne'], vBroad=[s['edge_a%d_vBroad' % a] for a in range(Na)], nStar=[s['edge_a%d_nStar' % a] for a in range(Na)],
                C=[s['edge_a%d_C' % a] for a in range(Na)], aDamp=[s['edge_a%d_aDamp' % a] for a in range(Na)])
    led = Ledger('%s five atoms' % lib.backend)
    for c, (T, ref) in enumerate(((raw['temperature'], falc), (s['edge_temperature'], edge))):
        check_setup_against_reference(led, data.atoms, prob, T, vB[c], aD[c], nStar[c], n[c], C[c], ref)
    led.report()
    return e, led


# ---- test 2: the collision spline against scipy, no reference needed ------------------------------------------------------
_EV = 1.60217733E-19
SPLINE_SIZES = (2, 4, 5, 7, 12, 80)


def _table(rng, n, kind):
    """non-uniform temperatures from >= 600 K; some tables span decades"""
    lo = rng.uniform(600.0, 3000.0)
    span = 10 ** rng.uniform(0.5, 3.0) if n > 4 else rng.uniform(3.0, 30.0)
    x = lo * span ** np.sort(np.concatenate([[0.0, 1.0], rng.uniform(0, 1, n - 2)]))
    y = 10 ** rng.uniform(-1.0, 1.0) * (x / x[0]) ** rng.uniform(-0.8, 0.8) * np.exp(rng.normal(0, 0.4, n))
    if kind == _capi.LSX_COLL_CI:
        y = y * 1e-16
    return x, y


def synthetic_atom():
    """8 levels (two ionisation stages), one line, Omega / CI / CE tables of 2, 4, 5, 7, 12 and 80 points on 18 distinct level
    pairs; the 7-point CE table's cubic dips below zero between its knots (the clamp runs), the 80-point CI spans 6 decades"""
    rng = np.random.default_rng(20261016)
    E = np.array([0.0, 1.5, 2.9, 4.1, 5.3, 6.2, 8.0, 9.5]) * _EV
    g = np.array([2.0, 4.0, 6.0, 2.0, 8.0, 4.0, 1.0, 3.0])
    stage = np.array([0, 0, 0, 0, 0, 0, 1, 1])
    pairs = [(i, j) for i in range(8) for j in range(i + 1, 8)]
    order = rng.permutation(len(pairs))
    colls, q = [], 0
    for kind in (_capi.LSX_COLL_OMEGA, _capi.LSX_COLL_CI, _capi.LSX_COLL_CE):
        for n in SPLINE_SIZES:
            i, j = pairs[order[q]]
            q += 1
            if kind == _capi.LSX_COLL_CI and n == 80:
                i, j = 0, 6                                   # 8 eV: dE / kT up to 230 at the lowest temperatures
                x = np.geomspace(700.0, 7e8, n) * np.exp(rng.uniform(-0.02, 0.02, n))
                y = 1e-16 * (x / 700.0) ** -0.3
            else:
                x, y = _table(rng, n, kind)
            if kind == _capi.LSX_COLL_CE and n == 7:
                y = y.copy()
                y[3] = -0.6 * y[3]                            # the cubic through a negative knot goes below zero around it
            colls.append(atomdata.CollisionData(int(kind), int(i), int(j), x, y))
    return atomdata.AtomData(weight=24.3, is_hydrogen=False, E_SI=E, g=g, stage=stage,
                             lines=[atomdata.LineData(0, 1, 1e8, 0.0)], collisions=colls)


def spline_temperatures(colls):
    """below, exactly at, one ulp either side of, between and above the knots of every table"""
    T = []
    for k in colls:
        x = np.asarray(k.temperature)
        T += [0.6 * x[0], x[-1] * 1.7, x[-1] * 40.0]
        T += list(x) + list(np.nextafter(x, 0.0)) + list(np.nextafter(x, np.inf))
        T += list(x[:-1] + (x[1:] - x[:-1]) * 0.37) + list(x[:-1] + (x[1:] - x[:-1]) * 0.81)
    return np.array(T)


def _one_atom_problem(atom, T, Ns=82):
    from toy import spec_problem
    ncol = -(-len(T) // Ns)
    prob, block = spec_problem([(len(atom.g), [('l', 0, 1, 0.2, 0.8)])], seed=5, Nspace=Ns, Nrays=1, Nspect=40, ncol=ncol, phi_compact=True)
    Tp = np.concatenate([T, np.full(ncol * Ns - len(T), 5000.0)]).reshape(ncol, Ns)
    return prob, block, Tp


def _lte_longdouble(atom, T, ne, nTotal):
    """atomic_set.py:105-145 (Debye lowering on) in long double"""
    ld = np.longdouble
    T, ne = T.astype(ld), ne.astype(ld)
    E, g, st = atom.E_SI.astype(ld), atom.g.astype(ld), np.asarray(atom.stage)
    c1 = (ld(K.HPlanck) / (2 * np.pi * ld(K.MElectron))) * (ld(K.HPlanck) / ld(K.KBoltzmann))
    c2 = np.sqrt(8 * np.pi / ld(K.KBoltzmann)) * (ld(K.QElectron) ** 2 / (4 * np.pi * ld(K.Epsilon0))) ** ld(1.5)
    dEion, cNe_T = c2 * np.sqrt(ne / T), ld(0.5) * ne * (c1 / T) ** ld(1.5)
    ns = np.zeros((len(g),) + T.shape, dtype=ld)
    ns[0] = 1
    for i in range(1, len(g)):
        nD = sum(range(st[i], st[i] + st[i] - st[0])) if st[i] > st[0] else 0
        ns[i] = g[i] / g[0] * np.exp(-(E[i] - E[0] - nD * dEion) / (ld(K.KBoltzmann) * T)) / cNe_T ** (st[i] - st[0])
    n0 = nTotal.astype(ld) / ns.sum(0)
    return ns * n0


def collision_spline_against_scipy(lib):
    """a synthetic atom whose Omega, CI and CE tables have 2, 4, 5, 7, 12 and 80 non-uniform points, evaluated below, at, one ulp
    either side of, between and above the knots: nStar against Saha-Boltzmann in long double, every rate entry against scipy's
    interp1d times the factors of collisional_rates.py:43-45, 68-70, 94-96 in long double, the clamp exact -> ledger"""
    atom = synthetic_atom()
    T = spline_temperatures(atom.collisions)
    prob, block, Tp = _one_atom_problem(atom, T)
    ncol, Ns = Tp.shape
    rng = np.random.default_rng(3)
    ne = 10 ** rng.uniform(12.0, 21.0, Tp.shape)
    nTot = np.full((ncol, 1, Ns), 1e15)
    e = Engine(prob, ncol, lib=lib)
    e.set_columns(0, block)
    e.set_atomic_data(atomdata.AtomicData([atom], 1.008, 4.003, 0.1))
    e.set_atmosphere(0, temperature=Tp, ne=ne, vturb=np.zeros_like(Tp), nHGround=np.full_like(Tp, 1e15), nTotal=nTot, lte_pops=True)
    nStar, n, C = e.get(_capi.LSX_NSTAR), e.get(_capi.LSX_N), e.get(_capi.LSX_C)
    led = Ledger('%s spline' % lib.backend)
    Tf, nef = Tp.reshape(-1), ne.reshape(-1)
    ns_ld = _lte_longdouble(atom, Tf, nef, nTot.reshape(-1))
    got_ns = np.moveaxis(nStar, 1, 0).reshape(len(atom.g), -1)
    led.check('nStar', got_ns, ns_ld.astype(np.float64), nstar_bar(atom.E_SI, Tf))
    assert np.array_equal(n, nStar)
    Nl = len(atom.g)
    got = np.moveaxis(C, 1, 0).reshape(Nl, Nl, -1)
    # expected: scipy's interpolant (float64, as the reference evaluates it) times the formulas' factors in long double
    ld = np.longdouble
    Cx = np.zeros((Nl, Nl, Tf.shape[0]), dtype=ld)
    B = np.zeros((Nl, Nl, Tf.shape[0]))
    for to, fr, c, bar in rate_contributions(atom, Tf, nef, ns_ld.astype(np.float64)):
        B[to, fr] += np.abs(c) * bar
    Tl, nel = Tf.astype(ld), nef.astype(ld)
    for k in atom.collisions:
        i, j = k.i, k.j
        v, _ = spline_terms(k.temperature, k.rates, Tf)
        v = v.astype(ld)
        if k.kind == _capi.LSX_COLL_OMEGA:
            down = ld(C0_OMEGA) * nel * v / (ld(atom.g[j]) * np.sqrt(Tl))
            Cx[i, j] += down; Cx[j, i] += down * ns_ld[j] / ns_ld[i]
        elif k.kind == _capi.LSX_COLL_CI:
            up = v * nel * np.exp(-(ld(atom.E_SI[j]) - ld(atom.E_SI[i])) / (ld(K.KBoltzmann) * Tl)) * np.sqrt(Tl)
            Cx[j, i] += up; Cx[i, j] += up * ns_ld[i] / ns_ld[j]
        else:
            down = v * nel * (ld(atom.g[i]) / ld(atom.g[j])) * np.sqrt(Tl)
            Cx[i, j] += down; Cx[j, i] += down * ns_ld[j] / ns_ld[i]
    neg = Cx < 0
    assert np.any(neg & (np.abs(Cx) > B)), 'the clamp is not reached'
    Cx[neg] = 0.0
    check_rates(led, 'C', got, Cx.astype(np.float64), B)
    led.report()
    return dict(nStar=got_ns, nStar_bar=nstar_bar(atom.E_SI, Tf), C=got, C_bar=B)


def spline_refusals(lib):
    """tables of 1 and 3 points and temperatures that do not strictly ascend are refused by lsx_set_atomic_data"""
    atom = synthetic_atom()
    prob, block, Tp = _one_atom_problem(atom, np.array([5000.0]))
    e = Engine(prob, 1, lib=lib)
    e.set_columns(0, block)
    base = atom.collisions[3]
    bad = [(np.array([3000.0]), np.array([1.0])),
           (np.array([3000.0, 5000.0, 9000.0]), np.array([1.0, 2.0, 1.5])),
           (np.array([3000.0, 5000.0, 4000.0, 9000.0]), np.ones(4)),
           (np.array([3000.0, 5000.0, 5000.0, 9000.0]), np.ones(4)),
           (np.array([9000.0, 7000.0, 5000.0, 3000.0, 1000.0]), np.arange(5.0) + 1),
           (np.array([3000.0, 2000.0]), np.ones(2))]
    for x, y in bad:
        colls = list(atom.collisions)
        colls[3] = atomdata.CollisionData(base.kind, base.i, base.j, x, y)
        a2 = atomdata.AtomData(atom.weight, False, atom.E_SI, atom.g, atom.stage, atom.lines, colls)
        with pytest.raises(_capi.LsxError, match='lsx_set_atomic_data'):
            e.set_atomic_data(atomdata.AtomicData([a2], 1.008, 4.003, 0.1))
    e.set_atomic_data(atomdata.AtomicData([atom], 1.008, 4.003, 0.1))          # the engine is still usable


# ---- test 3: the Voigt profile across the (a, v) plane ------------------------------------------------------------------------
VOIGT_LAMBDA0, VOIGT_VBROAD = 500.0, 4.0e3


def voigt_plane_inputs():
    """-> (wavelength [nm], aDamp [Ns]): a from 1e-8 to 1e3 (around 2 pi, where the pole term is dropped, and falc_all's largest
    6.14); |v| up to 3e3, around the pole-term cutoff 27 and the node-grid switch frac(2|v|) = 0.25, 0.75, both signs"""
    a = np.concatenate([np.geomspace(1e-8, 1e3, 34), [6.14, 2 * np.pi * (1 - 1e-9), 2 * np.pi, 2 * np.pi * (1 + 1e-9), 3.0, 9.0, 12.6]])
    v = [0.0, 1e-3, 0.05, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 5.0, 7.0, 15.0, 20.0, 26.9, 27.0 - 1e-9, 27.0, 27.0 + 1e-9, 27.1, 30.0,
         50.0, 100.0, 300.0, 1000.0, 2000.0, 3000.0]
    for base in (0.125, 0.375, 4.125, 10.375, 26.625, 26.875):
        v += [base - 1e-9, base, base + 1e-9]
    v = np.concatenate([v, np.geomspace(1e-2, 3e3, 60)])
    v = np.unique(np.concatenate([-v, v]))
    wl = VOIGT_LAMBDA0 * (1.0 + v * VOIGT_VBROAD / 2.99792458E+08)
    assert np.all(np.diff(wl) > 0)
    return wl, a


def voigt_plane(lib, with_vlos=False):
    """phi of a one-line problem whose samples cover the (a, v) plane, against scipy's wofz per entry; wphi against the float64
    trapezoid of that profile (tests/refprofile.py).  Bars: 4e-14 for the two Faddeeva evaluations (a float64 model of the library's
    rule is within 2.5e-14 of wofz on this plane) + 8 EPS |v d ln H / dv| (v's rounding on each side), 1e-13 on wphi -> ledger"""
    import refprofile
    from scipy.special import wofz
    from toy import spec_problem
    wl, a = voigt_plane_inputs()
    Ns = a.shape[0]
    prob, block = spec_problem([(2, [('l', 0, 1, 0.0, 1.0)])], seed=9, Nspace=Ns, Nrays=3, Nspect=wl.shape[0], ncol=1,
                               phi_compact=not with_vlos)
    prob.wavelength = np.array(wl)
    t = prob.trans[0]
    assert (t.Nblue, t.Nlambda) == (0, wl.shape[0])
    t.lambda0 = VOIGT_LAMBDA0
    block.phi = block.wphi = None
    vB = np.full(Ns, VOIGT_VBROAD) * np.linspace(1.0, 1.0 + 1e-6, Ns)       # not all equal: each depth its own v
    vlos = 2.5e3 * np.sin(np.linspace(0.0, 7.0, Ns)) if with_vlos else None
    e = Engine(prob, 1, lib=lib)
    e.set_columns(0, block)
    e.set_line_profiles(0, a[None, None], vB[None, None], None if vlos is None else vlos[None])
    phi, wphi = e.get(_capi.LSX_PHI)[0], e.get(_capi.LSX_WPHI)[0, 0]
    ref, wref = refprofile.profiles(wl, VOIGT_LAMBDA0, a, vB, np.zeros(Ns) if vlos is None else vlos, prob.muz, prob.wmu)
    vv = ((wl - VOIGT_LAMBDA0) * 2.99792458E+08)[:, None, None, None] / (vB * VOIGT_LAMBDA0)[None, None, None, :]
    if vlos is not None:
        vv = vv + (prob.muz[:, None, None] * np.array([-1.0, 1.0])[None, :, None]) * (vlos / vB)[None, None, None, :]
    z = vv + 1j * a[None, None, None, :]
    w = wofz(z)
    dlnH = np.abs(vv * (-2.0 * z * w).real / w.real)                      # v dH/dv / H, dw/dz = -2 z w + 2i / sqrt(pi)
    bar = 4e-14 + 8.0 * EPS * dlnH
    led = Ledger('%s voigt%s' % (lib.backend, ' vlos' if with_vlos else ''))
    if vlos is None:
        led.check('phi', phi, ref[:, 0, 0, :], bar[:, 0, 0, :])
    else:
        led.check('phi', phi, ref, np.broadcast_to(bar, ref.shape))
    led.check('wphi', wphi, wref, 1e-13)
    led.report()
    return dict(phi=phi, phi_bar=bar[:, 0, 0, :] if vlos is None else np.broadcast_to(bar, ref.shape), wphi=wphi, wphi_bar=1e-13)


def outputs_against_each_other(o1, o2, tag):
    """the outputs of collision_spline_against_scipy / voigt_plane of two libraries, each inside its bars around the
    high-precision reference: within twice those bars of each other, entry by entry (rates: the clamped zeros on both)"""
    led = Ledger(tag)
    for what in [k for k in o1 if not k.endswith('_bar')]:
        if what == 'C':
            check_rates(led, 'C', o1['C'], o2['C'], 2.0 * o1['C_bar'])
        else:
            led.check(what, o1[what], o2[what], 2.0 * np.asarray(o1[what + '_bar']))
    led.report()
