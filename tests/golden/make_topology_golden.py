#!/usr/bin/env python3
"""Generate tests/golden/topologies_*.npz: the reference's own Gamma loop (rh_method.py:565-745, formal_sol_gamma_matrices and
stat_equil of the UNMODIFIED reference, imported as tests/golden/make_golden.py imports it: same _refstubs, same avoid_recursion_eq
patch) on every made-up case of tests/topology_cases.py.

The loop reads nothing of the reference's set-up: Context, ComputationalAtom and ComputationalTransition only read attributes.  So
the three are made with __new__ and filled from the Problem / ColumnBlock the library is given (tests/toy.py), one column at a time:
  * transModel is a bare AtomicLine / AtomicContinuum instance (isLine, rh_method.py:150-155);
  * the given C arrives through one object in atomicModel.collisions whose compute_rates adds it, so the reference's own
    compute_collisions and its clamp run (rh_method.py:474-487);
  * compact profiles are broadcast to [lambda][mu][direction][depth], per-depth scattering over wavelength.
Protocol per case and golden column (topology_cases.golden_columns: the first and the last; the 700-depth cases keep one):
formal solutions 1-4 with a statistical equilibrium behind the 3rd and the 4th; t.Rij / t.Rji -- which the reference never zeroes --
are zeroed between calls 1 and 2, so that call 2's rates are those of ONE call with J-dagger = J of call 1 and the starting populations.
Kept: I, Gamma and dJ of every call, J of calls 1 and 4, n and dPops of both equilibria (dPops as the builtin max of
rh_method.py:742 leaves it), Rij / Rji of call 2, and topology_cases.input_digest of the column.  A column whose inputs an earlier
case holds bit for bit (the same seed with another column count) is written as its digest alone.  Numbers only; files are written
with fixed member time stamps, so a second run reproduces them byte for byte.

Usage:  python tests/golden/make_topology_golden.py [toy] [rs] [inst] [shallow] [bare] [dead] [all]        (default: all)
"""
import io
import os
import sys
import time
import warnings
import zipfile
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('LIGHTSPINNER_REF', '/root/reference')
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, '_refstubs'))
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

import atomic_model  # noqa: E402

_orig_eq = atomic_model.avoid_recursion_eq


def _compat_eq(a, b):
    if isinstance(a, np.ndarray):
        if not isinstance(b, np.ndarray) or a.shape != b.shape:
            return False
    return _orig_eq(a, b)


atomic_model.avoid_recursion_eq = _compat_eq

from atomic_model import AtomicLine, AtomicContinuum  # noqa: E402
from rh_method import Context, ComputationalAtom, ComputationalTransition  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository: lightspinner_amd.problem (pure Python)
sys.path.insert(0, os.path.dirname(HERE))                       # tests/: the table of cases
import topology_cases as tc  # noqa: E402

FILE_BUDGET = 900_000          # bytes per fixture file (compressed members), below the limit of a committed file


class _Bag:
    pass


class _GivenRates:
    """the column's collisional rates, handed to compute_collisions the way a model's own terms are"""

    def __init__(self, C):
        self.C = C

    def compute_rates(self, atmos, nStar, Cmat):
        Cmat += self.C


def reference_context(prob, block, col):
    """the reference's Context of column `col`, hand-filled"""
    Ns, Nrays = prob.Nspace, prob.Nrays
    atmos = _Bag()
    atmos.Nspace, atmos.Nrays = Ns, Nrays
    atmos.muz, atmos.wmu = np.array(prob.muz), np.array(prob.wmu)
    atmos.height, atmos.temperature = np.array(block.height[col]), np.array(block.temperature[col])
    spect = _Bag()
    spect.wavelength = np.array(prob.wavelength)
    bg = _Bag()
    bg.chi, bg.eta = np.array(block.bg_chi[col]), np.array(block.bg_eta[col])
    sca = np.array(block.bg_sca[col])
    bg.sca = sca if prob.sca_per_lambda else np.broadcast_to(sca[None, :], (prob.Nspect, Ns)).copy()
    atoms = []
    for a, nl in enumerate(prob.Nlevel):
        lo, lo2 = int(prob.lev_off[a]), int(prob.lev2_off[a])
        atom = ComputationalAtom.__new__(ComputationalAtom)
        atom.atmos, atom.spect = atmos, spect
        atom.atomicModel = _Bag()
        atom.atomicModel.name = prob.atom_names[a]
        atom.atomicModel.collisions = [_GivenRates(np.array(block.C[col, lo2:lo2 + nl * nl]).reshape(nl, nl, Ns))]
        atom.nStar = np.array(block.nStar[col, lo:lo + nl])
        atom.n = np.array(block.n[col, lo:lo + nl])
        atom.nTotal = np.array(block.nTotal[col, a])
        atom.Nlevel = nl
        atom.Gamma = np.zeros((nl, nl, Ns))
        atom.C = np.zeros((nl, nl, Ns))
        atom.trans = []
        for kr, t in enumerate(prob.trans):
            if t.atom != a:
                continue
            ct = ComputationalTransition.__new__(ComputationalTransition)
            ct.atom = atom
            ct.wavelength = spect.wavelength[t.Nblue:t.Nblue + t.Nlambda].copy()
            ct.i, ct.j, ct.Nblue = int(t.i), int(t.j), int(t.Nblue)
            ct.active = prob.active[kr].astype(np.bool_)
            ct.gij = None
            ct.Rij, ct.Rji = np.zeros(Ns), np.zeros(Ns)
            ct.kr = kr
            if t.is_line:
                ct.transModel = AtomicLine.__new__(AtomicLine)
                ct.Aji, ct.Bji, ct.Bij, ct.lambda0 = float(t.Aji), float(t.Bji), float(t.Bij), float(t.lambda0)
            else:
                ct.transModel = AtomicContinuum.__new__(AtomicContinuum)
                ct.alpha = np.array(t.alpha, dtype=np.float64)
            atom.trans.append(ct)
        atom.Ntrans = len(atom.trans)
        atoms.append(atom)
    # the profile store follows prob.lines (the lines of all atoms in transition order)
    phi_off, line_idx = 0, 0
    by_kr = {ct.kr: ct for atom in atoms for ct in atom.trans}
    for kr, t in enumerate(prob.trans):
        if not t.is_line:
            continue
        ct = by_kr[kr]
        p = np.array(block.phi[col, phi_off:phi_off + t.Nlambda])
        ct.phi = np.broadcast_to(p[:, None, None, :], (t.Nlambda, Nrays, 2, Ns)).copy() if prob.phi_compact else p
        ct.wphi = np.array(block.wphi[col, line_idx])
        phi_off += t.Nlambda
        line_idx += 1
    for atom in atoms:
        atom.setup_wavelength(0)
    ctx = Context.__new__(Context)
    ctx.atmos, ctx.spect, ctx.background = atmos, spect, bg
    ctx.activeAtoms = atoms
    ctx.J = np.zeros((prob.Nspect, Ns))
    ctx.I = np.zeros((prob.Nspect, Nrays))
    return ctx


def run_column(prob, block, col):
    ctx = reference_context(prob, block, col)
    d = {'digest': tc.input_digest(prob, block, col)}
    trans = sorted((ct for atom in ctx.activeAtoms for ct in atom.trans), key=lambda ct: ct.kr)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        for it in (1, 2, 3, 4):
            if it == 2:
                for ct in trans:
                    ct.Rij.fill(0.0)
                    ct.Rji.fill(0.0)
            dJ = ctx.formal_sol_gamma_matrices()
            tag = 'fs%d_' % it
            d[tag + 'I'] = ctx.I.copy()
            d[tag + 'dJ'] = np.float64(dJ)
            d[tag + 'Gamma'] = np.concatenate([atom.Gamma.reshape(atom.Nlevel ** 2, prob.Nspace) for atom in ctx.activeAtoms])
            if it in (1, 4):
                d[tag + 'J'] = ctx.J.copy()
            if it == 2:
                d[tag + 'Rij'] = np.stack([ct.Rij for ct in trans]) if trans else np.zeros((0, prob.Nspace))
                d[tag + 'Rji'] = np.stack([ct.Rji for ct in trans]) if trans else np.zeros((0, prob.Nspace))
            if it >= 3:
                dP = ctx.stat_equil()
                d['se%d_dPops' % it] = np.float64(dP)
                d['se%d_n' % it] = np.concatenate([atom.n for atom in ctx.activeAtoms])
    return d


_SEEN = {}          # name -> the columns whose inputs an earlier case of the table has already (same digest): only the digest is written


def run_case(name):
    t0 = time.time()
    prob, block = tc.build(name)
    out = {}
    for col in tc.golden_columns(name, block.ncol):
        if col in _SEEN[name]:
            out['%s/c%d/digest' % (name, col)] = tc.input_digest(prob, block, col)
            continue
        for k, v in run_column(prob, block, col).items():
            out['%s/c%d/%s' % (name, col, k)] = v
    print('%-55s %5.1f s' % (name, time.time() - t0), flush=True)
    return out


def find_repeats():
    """columns that an earlier case of the table holds already, bit for bit (the same seed with another column count gives the same
    first column): the fixture keeps their results once, tests find them by digest"""
    seen = set()
    for name in tc.NAMES:
        prob, block = tc.build(name)
        _SEEN[name] = set()
        for col in tc.golden_columns(name, block.ncol):
            dg = tc.input_digest(prob, block, col).tobytes()
            if dg in seen:
                _SEEN[name].add(col)
            seen.add(dg)


def _member(arr):
    buf = io.BytesIO()
    np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
    return buf.getvalue()


def write_family(fam, d):
    """the family's arrays into topologies_<family>_<k>.npz, in order, a new file whenever the next member would take the file over
    FILE_BUDGET; member time stamps fixed (numpy's savez stamps the clock)"""
    for f in os.listdir(HERE):
        if f.startswith('topologies_%s_' % fam) and f.endswith('.npz'):
            os.remove(os.path.join(HERE, f))
    files, used = [[]], 0
    for key, arr in d.items():
        raw = _member(arr)
        size = len(zlib.compress(raw, 6)) + len(key) * 2 + 120
        if files[-1] and used + size > FILE_BUDGET:
            files.append([])
            used = 0
        files[-1].append((key, raw))
        used += size
    for k, members in enumerate(files):
        path = os.path.join(HERE, 'topologies_%s_%02d.npz' % (fam, k))
        with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED, compresslevel=6) as z:
            for key, raw in members:
                zi = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
                zi.compress_type = zipfile.ZIP_DEFLATED
                zi.external_attr = 0o644 << 16
                z.writestr(zi, raw, compresslevel=6)
        print('wrote %s (%.1f kB)' % (path, os.path.getsize(path) / 1e3), flush=True)


if __name__ == '__main__':
    import multiprocessing as mp
    what = sys.argv[1:] or ['all']
    fams = tc.FAMILIES if 'all' in what else what
    assert all(f in tc.FAMILIES for f in fams), fams
    names = [n for n in tc.NAMES if tc.family(n) in fams]
    t0 = time.time()
    find_repeats()
    nproc = max(1, min(8, len(os.sched_getaffinity(0)), len(names)))
    with mp.get_context('fork').Pool(nproc) as pool:
        results = pool.map(run_case, names, chunksize=1)
    for fam in fams:
        d = {}
        for n, r in zip(names, results):
            if tc.family(n) == fam:
                d.update(r)
        write_family(fam, d)
    print('done in %.1f s' % (time.time() - t0), flush=True)
