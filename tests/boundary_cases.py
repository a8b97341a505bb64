"""What the tests of the radiation boundary conditions share (include/lsx_hip_boundary.h; tests/test_boundary_host.py,
tests/test_boundary.py) with the generator of their fixture (tests/golden/make_boundary_golden.py): the cases -- named cases of
tests/topology_cases.py, the smallest shapes at which each mapping can go wrong --, the (lower, upper) combinations, the intensities
handed over where a kind is GIVEN, and the start value of a ray as the table of the header states it.

The fixture tests/golden/boundary_*.npz is the reference's own Gamma loop with rh_method.piecewise_linear_1d replaced by start_value()
in front of the reference's own formal_solver.piecewise_1d_impl.  The protocol per case, combination and golden column: two formal
solutions, J-dagger = 0 and then J-dagger = J of call 1, the rates zeroed between them.  Kept: I, Gamma and dJ of both calls, J of call
1, Rij / Rji of call 2, the input digest."""
import glob
import hashlib
import os
import zipfile

import numpy as np

import topology_cases as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

ZERO, THERMALISED, GIVEN = 0, 1, 2
LETTER = {'Z': ZERO, 'T': THERMALISED, 'G': GIVEN}
COMBOS = ['ZZ', 'TT', 'GG', 'ZG', 'GZ']          # (lower, upper); the default TZ is not stored: it is the topology fixture
DEFAULT = 'TZ'

CASES = [
    'rs-see21-Nra5-Nsp3-Nsp60-nco36',                 # ray-serial, the shortest column, ragged last group
    'rs-see13-Nra5-Nsp41-Nsp120-nco34-mul3',          # ray-serial, odd depth count
    'toy-see5-Nra2-Nsp5-Nsp40-nco40',                 # one ray per lane, per-class launches
    'toy-see7-Nra8-Nsp21-Nsp48-nco2',                 # fused small-batch, all 64 lanes
    'toy-see14-Nra5-Nsp41-Nsp120-nco3-mul3',          # fused, linked continua
    'toy-see9-Nra3-Nsp700-Nsp30-nco2',                # the generic instance; one column in the fixture
    'shallow-3',                                      # shallow columns, two atoms
    'inst-two_atoms',
]
assert all(n in tc.TABLE for n in CASES)
DEFAULT_KEYS = ['fs1_I', 'fs1_J', 'fs1_Gamma', 'fs2_I', 'fs2_Gamma']     # what the default kinds are held to, bit for bit
KEYS = ['fs1_I', 'fs1_Gamma', 'fs1_dJ', 'fs1_J', 'fs2_I', 'fs2_Gamma', 'fs2_dJ', 'fs2_Rij', 'fs2_Rji']


def sha(a):
    """SHA-256 of an array's shape and bytes, as uint8 [32]"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.frombuffer(hashlib.sha256(str(a.shape).encode() + a.tobytes()).digest(), dtype=np.uint8).copy()


def kinds(combo):
    return LETTER[combo[0]], LETTER[combo[1]]


def planck(temp, wav):
    """B_nu(T) at wavelength wav [nm], SI (the reference's utils.planck: the constants of its constants.py)"""
    HC, KB, NM = 6.6260755E-34 * 2.99792458E+08, 1.380658E-23, 1.0E-09
    hc_Tkla = HC / (KB * NM * wav) / temp
    twohnu3_c2 = (2.0 * HC) / (NM * wav)**3
    return twohnu3_c2 / (np.exp(hc_Tkla) - 1.0)


def given_arrays(prob, block, col):
    """-> (I_lower, I_upper) [Nspect][Nrays] of column `col`: angle and wavelength dependent
         I_lower[la][m] = 0.7 B(T[-1], lambda) (0.4 + 0.6 mu_m),   I_upper[la][m] = 0.3 B(6000 K, lambda)"""
    wav = np.asarray(prob.wavelength, dtype=np.float64)
    mu = np.asarray(prob.muz, dtype=np.float64)
    lo = (0.7 * planck(float(block.temperature[col][-1]), wav))[:, None] * (0.4 + 0.6 * mu)[None, :]
    up = np.broadcast_to((0.3 * planck(6000.0, wav))[:, None], (wav.shape[0], mu.shape[0]))
    return np.ascontiguousarray(lo), np.ascontiguousarray(up)


def start_value(kind, to_obs, given, muz, z, temperature, wav, chi, planck_fn=planck):
    """the value a ray starts with (include/lsx_hip_boundary.h): to_obs = up-going, from the lower end.  THERMALISED at the lower end
    is formal_solver.py:203-207, at the upper end its mirror image"""
    if kind == ZERO:
        return 0.0
    if kind == GIVEN:
        return float(given)
    k0, k1 = (len(z) - 1, len(z) - 2) if to_obs else (0, 1)
    dtau_uw = (1.0 / muz) * (chi[k0] + chi[k1]) * 0.5 * np.abs(z[k0] - z[k1])
    Bnu = planck_fn(np.array([temperature[k1], temperature[k0]]), wav)
    return Bnu[1] - (Bnu[0] - Bnu[1]) / dtau_uw


def set_on(engine, combo, prob, block, cols=None):
    """put combination `combo` with given_arrays on every column of a loaded engine (cols: which columns of `block` the engine's are)"""
    cols = range(block.ncol) if cols is None else cols
    lo, up = kinds(combo)
    arr = [given_arrays(prob, block, c) for c in cols]
    engine.set_boundary(lo, up, I_lower=np.stack([a[0] for a in arr]) if lo == GIVEN else None,
                        I_upper=np.stack([a[1] for a in arr]) if up == GIVEN else None)


def library_engine(lib, prob, block, prof):
    """an engine whose line profiles the library builds itself from `prof` (aDamp, vBroad, vlos: tests/final_pass_cases.py,
    library_profiles), so that the passes at other angles and wavelengths can rebuild them"""
    import dataclasses
    from lightspinner_amd import synth
    from lightspinner_amd.problem import Engine
    e = Engine(prob, block.ncol, lib=lib)
    synth.load_columns(e, dataclasses.replace(block, phi=None, wphi=None), prof)
    return e


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------
_index = {}


def fixture_index():
    if not _index:
        for path in sorted(glob.glob(os.path.join(GOLDEN, 'boundary_*.npz'))):
            with zipfile.ZipFile(path) as z:
                for m in z.namelist():
                    assert m.endswith('.npy') and m[:-4] not in _index, (path, m)
                    _index[m[:-4]] = path
    return _index


def read(key):
    with np.load(fixture_index()[key]) as z:
        return z[key]


def results(name, combo, cols):
    """{key: array stacked over the golden columns} of the fixture, with the digests"""
    out = {k: np.stack([read('%s/%s/c%d/%s' % (name, combo, c, k)) for c in cols]) for k in KEYS}
    out['digest'] = [read('%s/c%d/digest' % (name, c)) for c in cols]
    return out
