"""One table of the made-up topologies: every case that tests/test_toy_topologies.py, tests/test_instances_gpu.py and the ledger run
HIP against the oracle, under a stable name, with build(name) -> (prob, block).

The same table is what tests/golden/make_topology_golden.py drives the reference's own loop on (rh_method.py:565-745, the unmodified
formal_sol_gamma_matrices / stat_equil on hand-filled objects): tests/golden/topologies_*.npz hold the reference's I, J, Gamma, n,
monitors and rates of the golden columns of every case here, tests/test_topologies_reference_host.py pins the oracle on them and
tests/test_topologies_reference.py the HIP kernels.  input_digest() ties a fixture to the arrays it was computed from."""
import hashlib

import numpy as np

from toy import spec_problem, toy_problem

# ---- tests/test_toy_topologies.py ----------------------------------------------------------------------------------------------------------------
CASES = [
    dict(seed=1),                                                     # 3 rays, 37 depths, chained continua
    dict(seed=2, Nrays=1, Nspace=20, Nspect=70),                      # 64 wavelengths per wavefront
    dict(seed=3, Nrays=5, Nspace=82, Nspect=130, sca_per_lambda=True),
    dict(seed=4, phi_compact=True, chain=False),
    dict(seed=5, Nrays=2, Nspace=5, Nspect=40, ncol=40),              # shortest useful column; >= 32 columns: per-class launches
    dict(seed=6, Nrays=7, Nspace=33, Nspect=55, ncol=33),
    dict(seed=7, Nrays=8, Nspace=21, Nspect=48, ncol=2),              # 8 wavelengths per wavefront, all 64 lanes used
    dict(seed=8, Nrays=3, Nspace=700, Nspect=30, ncol=33),            # deep column: the operand table no longer fits LDS -> generic instance
    dict(seed=9, Nrays=3, Nspace=700, Nspect=30, ncol=2),             # same through the fused small-batch launch
    # regular bound-free sets on even tile widths: the column-mapped epilogue (k_fast_gamma_cols), with linked continua
    dict(seed=10, Nrays=4, Nspace=45, Nspect=100, ncol=34, chain=False),
    dict(seed=11, Nrays=5, Nspace=82, Nspect=140, ncol=3, chain=False),
    dict(seed=12, Nrays=8, Nspace=31, Nspect=64, ncol=33, chain=False, phi_compact=True),
    # multiplets under linked continua: three per-ray slots (the <3, 3, linked> instance) and four (no such instance: the plan
    # files the tile under the generic linked kernel), through the per-class launches (>= 32 columns) and the fused launch
    dict(seed=13, Nrays=5, Nspace=41, Nspect=120, ncol=34, multiplet=3),
    dict(seed=14, Nrays=5, Nspace=41, Nspect=120, ncol=3, multiplet=3),
    dict(seed=15, Nrays=5, Nspace=41, Nspect=120, ncol=34, multiplet=4),
    dict(seed=16, Nrays=5, Nspace=41, Nspect=120, ncol=3, multiplet=4),
    dict(seed=17, Nrays=3, Nspace=30, Nspect=150, ncol=33, multiplet=4, phi_compact=True),
]

RS_CASES = [
    dict(seed=11, Nrays=5, Nspace=82, Nspect=140, ncol=33, chain=False),        # 33 columns: six full groups of five and one of three
    dict(seed=13, Nrays=5, Nspace=41, Nspect=120, ncol=34, multiplet=3),        # odd depth count: the two directions meet in one step
    dict(seed=15, Nrays=5, Nspace=41, Nspect=120, ncol=37, multiplet=4),        # four-line multiplets (generic class beside the ray-serial ones)
    dict(seed=21, Nrays=5, Nspace=3, Nspect=60, ncol=36),                       # the shortest column the rule allows
    dict(seed=22, Nrays=5, Nspace=30, Nspect=90, ncol=41, phi_compact=True),    # ray-independent profiles
]

# ---- tests/instance_cases.py: (topology, ncol, Nspace, phi_compact): >= 32 columns so that the per-class launches run (one kernel
# instance per tile class); ragged column groups for the five-column wavefronts of the ray-serial kernel; odd and even depth counts
INSTANCE_CASES = [
    ('stages1', 33, 31, False), ('stages2', 34, 40, False), ('stages3', 36, 33, False), ('multi_up', 37, 38, False),
    ('two_atoms', 33, 35, False), ('linked_up', 34, 36, False), ('linked_low', 35, 29, True), ('mixed', 33, 34, False),
    ('triplet', 32, 30, False), ('crowd', 33, 27, False),
]

# ---- tests/test_instances_gpu.py: the shallowest columns, and three atoms of which the middle one has collisions only
SHALLOW_DEPTHS = [3, 4, 5, 6]
SHALLOW_NCOL = 33
BARE_ATOMS = [(3, [('l', 0, 1, 0.1, 0.5), ('c', 1, 2, 0.0, 0.3)]), (2, []), (3, [('l', 0, 2, 0.4, 0.9), ('c', 0, 2, 0.0, 0.2)])]
BARE_NCOL = [3, 40]
# ---- tests/context_cases.py: the level that nothing populates (0 / 0 in the second statistical equilibrium, rh_method.py:741-742)
DEAD_LEVEL = dict(seed=11, ncol=3, dead_level=True)


def kw_id(kw):
    """the parametrisation id of a toy_problem case (what tests/test_toy_topologies.py shows)"""
    return '-'.join('%s%s' % (a[:3], b) for a, b in kw.items())


def _table():
    t = {}
    for kw in CASES:
        t['toy-' + kw_id(kw)] = ('toy', kw)
    for kw in RS_CASES:
        t['rs-' + kw_id(kw)] = ('toy', kw)
    for case in INSTANCE_CASES:
        t['inst-' + case[0]] = ('inst', case)
    for Ns in SHALLOW_DEPTHS:
        t['shallow-%d' % Ns] = ('inst', ('two_atoms', SHALLOW_NCOL, Ns, False))
    for ncol in BARE_NCOL:
        t['bare-%d' % ncol] = ('bare', ncol)
    t['dead-level'] = ('toy', DEAD_LEVEL)
    return t


TABLE = _table()
NAMES = list(TABLE)
FAMILIES = ['toy', 'rs', 'inst', 'shallow', 'bare', 'dead']      # the part of a name in front of its first '-': one set of fixture files each


def family(name):
    return name.split('-', 1)[0]


def build(name):
    """-> (prob, block) of the case, every column"""
    kind, arg = TABLE[name]
    if kind == 'toy':
        return toy_problem(**arg)
    if kind == 'inst':
        import instance_cases as ic
        return ic.build(*arg)
    return spec_problem(BARE_ATOMS, seed=5, Nspace=30, Nrays=5, Nspect=200, ncol=arg)


def golden_columns(name, ncol):
    """the columns the fixture holds the reference's results for: the first, and the last (the ragged last group of the ray-serial
    wavefronts); the 700-depth cases keep one column (the size of a committed fixture)"""
    if ncol == 1 or TABLE[name][0] == 'toy' and TABLE[name][1].get('Nspace', 0) >= 700:
        return [0]
    return [0, ncol - 1]


def input_digest(prob, block, col):
    """SHA-256 over everything the loop reads of column `col`: its input arrays, the grids, the quadrature and the transition table"""
    h = hashlib.sha256()

    def put(x, dtype=np.float64):
        a = np.ascontiguousarray(x, dtype=dtype)
        h.update(('%s%s' % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    put([prob.Nspace, prob.Nrays, prob.Nspect, int(prob.sca_per_lambda), int(prob.phi_compact)] + list(prob.Nlevel), np.int64)
    for x in (prob.wavelength, prob.muz, prob.wmu):
        put(x)
    put(prob.active, np.uint8)
    for t in prob.trans:
        put([t.atom, int(t.is_line), t.i, t.j, t.Nblue, t.Nlambda], np.int64)
        put([t.Aji, t.Bji, t.Bij, t.lambda0])
        if not t.is_line:
            put(t.alpha)
    for k in ('height', 'temperature', 'nStar', 'nTotal', 'n', 'C', 'bg_chi', 'bg_eta', 'bg_sca', 'phi', 'wphi'):
        put(getattr(block, k)[col])
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()
