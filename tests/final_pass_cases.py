"""Shared cases of the final-pass shape tests (tests/test_final_pass_shapes_host.py, tests/test_final_pass_shapes.py): small made-up
problems (tests/toy.py) on which the four read-only entries -- lsx_hip_radiative_rates, lsx_hip_emergent_rays, lsx_hip_depth_rays,
lsx_hip_spectrum -- run off the FALC shape (five rays: 12 wavelengths per tile, 82 depths, the reference's atoms).

What the table covers:
  * ray counts 1, 2, 3, 4, 6, 7, 8, 9, 11 and 64: lsx_rates.hip walks the context's rays in groups of five (`take = min(5, Nrays - m0)`),
    so these reach k_rates_pass<NM, PAR> for every NM as the FIRST group of a call (which starts the work arrays) and as a LATER
    group (which reads them back and adds), and the tile widths L = 64 / Nrays = 64, 32, 21, 16, 10, 9, 8, 7, 5 and 1 with ragged
    last tiles.  GROUPS states the decomposition per case; `check_group_coverage` asserts it against the problems and that nothing
    is missing;
  * the toy topologies: chained and unchained continua, multiplets of three and four lines under linked continua, a continua-only
    atom, a dead level (n == 0 exactly after a statistical equilibrium), scattering per wavelength, ray-dependent and compact
    profiles, and one problem without continua (the kernels' E == NULL / nsr == NULL branches);
  * odd and even depth counts between 20 and 45, and columns of 3, 4 and 5 depths.  The shallow ones are the DEEPEST points of a
    37-depth toy column (`deepest`), not toy_problem(Nspace=3): the thermalised lower boundary of so thin a slab at the top of the
    atmosphere gives negative intensities under the linear rule, and a relative bar on a J or a rate that changes sign says nothing;
  * 3 columns, and 7 in one case (chunking under a work cap, column sub-ranges).

Nothing here reads the reference.  tests/test_final_pass_shapes_host.py asserts on the oracle alone that every case is well posed
(positive J, I and rates; bounds that are nowhere vacuous): that is what lets the GPU tests use the FALC tests' bars as they are."""
import dataclasses
import functools

import numpy as np

import rays_cases as rc
import spectrum_cases as sc
from toy import spec_problem, toy_problem
from lightspinner_amd.problem import ColumnBlock

SOLVERS = ('linear', 'parabolic')
GROUP = 5                          # rays a lane carries at a time in lsx_rates.hip
VACUITY_CAP = 1e-9                 # no entry's bound (BASE |x| + K |x(+1) - x(-1)|) may be wider than this, relative


# ---- profile inputs and wanted wavelengths for the made-up problems ----------------------------------------------------------------
def made_up_profiles(prob, block):
    """profile inputs for the made-up problems of tests/toy.py (their lines are tens of nm wide)"""
    depth = np.linspace(0.0, 1.0, prob.Nspace)
    aD = np.tile(0.02 * (1.0 + depth), (block.ncol, prob.Nlines, 1))
    vB = np.tile(6.0e6 * (1.0 + 0.5 * depth), (block.ncol, prob.Natoms, 1))
    vl = 2.0e5 * np.sin(3.0 * depth[None, :] + np.arange(block.ncol)[:, None])
    return aD, vB, vl


def made_up_wanted(prob):
    lam = prob.wavelength
    return np.unique(np.concatenate([0.5 * (lam[1:] + lam[:-1])[::4], lam[::37], [0.8 * lam[0], 1.2 * lam[-1]]]))


def given_background(prob, block, w):
    """a background of the caller's that is NOT the interpolated one: the rule's values times a smooth factor"""
    f = 1.0 + 0.01 * np.sin(np.arange(w.shape[0]))[:, None]
    out = [sc.interp_rule(prob.wavelength, block.bg_chi, w) * f, sc.interp_rule(prob.wavelength, block.bg_eta, w) * f]
    if prob.sca_per_lambda:
        out.append(sc.interp_rule(prob.wavelength, block.bg_sca, w) * f)
    return tuple(out)


def library_profiles(prob, block):
    """-> (block without profile arrays, profile inputs): the context builds its own profiles (lsx_set_line_profiles), so they can
    be rebuilt at other angles and wavelengths.  A phi_compact context takes no velocity."""
    aD, vB, vl = made_up_profiles(prob, block)
    return dataclasses.replace(block, phi=None, wphi=None), (aD, vB, None if prob.phi_compact else vl)


def rays_inputs(prob, block):
    """what the emergent-ray and depth tests load: a compact context's own arrays are ray independent and served as they are; a
    ray-dependent context gets made-up profile inputs"""
    return (block, None) if prob.phi_compact else library_profiles(prob, block)


# ---- builders -----------------------------------------------------------------------------------------------------------------------
def deepest(prob, block, m):
    """the deepest m points of every column: the last axis of every array of the block"""
    p2 = dataclasses.replace(prob, Nspace=m)
    fields = {f.name: getattr(block, f.name) for f in dataclasses.fields(ColumnBlock)}
    b2 = ColumnBlock(**{k: (None if v is None else np.ascontiguousarray(v[..., -m:])) for k, v in fields.items()})
    return p2, b2.validate(p2)


def _toy(**kw):
    return lambda: toy_problem(**kw)


def _deep(m, **kw):
    def build():
        prob, block = toy_problem(Nspace=37, **kw)
        return deepest(prob, block, m)
    return build


def _lines_only():
    return spec_problem([(3, [('l', 0, 1, .1, .6), ('l', 0, 2, .4, .9)])], seed=41, Nspace=29, Nrays=6, Nspect=60, ncol=3)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    builder: object
    groups: tuple                  # the launches of one lsx_hip_radiative_rates call: rays per k_rates_pass launch, in order
    state: str = 'mali'            # 'mali': rays_cases.mali (five formal solutions, the last two with a statistical equilibrium);
                                   # 'two_fs': two formal solutions (the shallow columns, as the existing three-depth tests)


CASES = (
    # 20 - 45 depths, odd and even; three columns unless said
    Case('r1-sca',        _toy(seed=31, Nrays=1, Nspace=20, Nspect=70, sca_per_lambda=True), (1,)),            # L = 64, ragged tile of 6
    Case('r2-unchained',  _toy(seed=32, Nrays=2, Nspace=33, Nspect=90, chain=False, phi_compact=True), (2,)),
    Case('r3-dead-level', _toy(seed=33, Nrays=3, Nspace=37, Nspect=90, dead_level=True), (3,)),
    Case('r4-multiplet4', _toy(seed=34, Nrays=4, Nspace=45, Nspect=100, multiplet=4), (4,)),
    Case('r6-chained',    _toy(seed=35, Nrays=6, Nspace=24, Nspect=95), (5, 1)),                                # L = 10
    Case('r7-multiplet3', _toy(seed=36, Nrays=7, Nspace=33, Nspect=75, multiplet=3), (5, 2)),                   # L = 9
    Case('r8-compact',    _toy(seed=37, Nrays=8, Nspace=30, Nspect=90, chain=False, phi_compact=True), (5, 3)),  # L = 8
    Case('r9-sca',        _toy(seed=38, Nrays=9, Nspace=21, Nspect=80, sca_per_lambda=True), (5, 4)),            # L = 7
    Case('r11-7columns',  _toy(seed=39, Nrays=11, Nspace=41, Nspect=120, ncol=7), (5, 5, 1)),                    # L = 5
    Case('r64',           _toy(seed=47, Nrays=64, Nspace=40, Nspect=40, chain=False, phi_compact=True), (5,) * 12 + (4,)),   # L = 1
    Case('lines-only',    _lines_only, (5, 1)),                                                                  # any_cont == false
    # the deepest 3, 4 and 5 points of a 37-depth column
    Case('deepest3-r7',   _deep(3, seed=42, Nrays=7, Nspect=60), (5, 2), 'two_fs'),
    Case('deepest4-r8',   _deep(4, seed=43, Nrays=8, Nspect=60, phi_compact=True), (5, 3), 'two_fs'),
    Case('deepest5-r2',   _deep(5, seed=44, Nrays=2, Nspect=60, multiplet=3), (2,), 'two_fs'),
)
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(BY_NAME)
RATES_PARAMS = [(c.name, s) for c in CASES for s in SOLVERS]          # every case under both rules
SEVEN_COLUMNS = 'r11-7columns'
FROZEN = 'r8-compact'
QUADRATURE = ('r1-sca', 'r7-multiplet3', 'r8-compact', 'r64')          # 1, 7, 8 and 64 rays
# the contexts of the depth and spectrum tests (name, rules)
DEPTH = (('r7-multiplet3', SOLVERS), ('r8-compact', ('linear',)), ('r1-sca', ('linear',)))
SPECTRUM = DEPTH + (('lines-only', ('linear',)),)


@functools.lru_cache(maxsize=None)
def build(name):
    """-> (prob, block) of a case; shared between the tests, which leave it unchanged"""
    prob, block = BY_NAME[name].builder()
    for f in dataclasses.fields(ColumnBlock):
        a = getattr(block, f.name)
        if a is not None:
            a.setflags(write=False)
    return prob, block


def reach_state(engine, case):
    if case.state == 'mali':
        rc.mali(engine)
    else:
        engine.formal_sol_gamma()
        engine.formal_sol_gamma()


def walk_in_groups(Nrays):
    """the launches lsx_hip_radiative_rates makes for a context of Nrays rays (lsx_rates.hip: take = min(group, Nrays - m0))"""
    out, m0 = [], 0
    while m0 < Nrays:
        out.append(min(GROUP, Nrays - m0))
        m0 += out[-1]
    return tuple(out)


def instances_reached(params=None):
    """-> {(NM, parabolic, first group of a call): [case names]} over `params` [(case name, rule)]"""
    seen = {}
    for name, solver in (RATES_PARAMS if params is None else params):
        for q, nm in enumerate(BY_NAME[name].groups):
            seen.setdefault((nm, solver == 'parabolic', q == 0), []).append(name)
    return seen


def check_group_coverage(params=None):
    """the stated decomposition of every case is the one its problem gives, and over the table every NM = 1 .. 5 occurs as a first
    group and as a later group under either rule: all ten k_rates_pass<NM, PAR> with `first` set and with the read-back branch"""
    for c in CASES:
        prob, _ = build(c.name)
        assert sum(c.groups) == prob.Nrays and c.groups == walk_in_groups(prob.Nrays), (c.name, c.groups, prob.Nrays)
    seen = instances_reached(params)
    missing = [(nm, 'parabolic' if par else 'linear', 'first' if first else 'later')
               for nm in range(1, GROUP + 1) for par in (False, True) for first in (True, False) if (nm, par, first) not in seen]
    assert not missing, 'no case reaches k_rates_pass<NM, rule> as a first / later group: %s' % missing
    return seen
