"""The ledger of the compiled instances of the fast-continuum epilogue -- the kernels that run behind the sweep and write the Gamma
entries of the fast (bound-free) continua: k_fast_gamma<LP, NT, SEG> (row mapped, 18 instances, on its two paths: "simple" tiles
with three running sums per atom, and the per-thread level cells in front of the staged operands), k_fast_gamma_cols<NLC, NPC>,
k_fast_gamma_cols_big<NLC> and k_fast_prepass<SEG>.  This module is the shared data of the two sides:

  tests/test_epilogue_ledger.py    (CPU)  walks the instance lists of lsx_plan.h (lsx_plan_epilogue_instances) and the launch shapes the
                                          product's planner gives the problems below (lsx_plan_epilogue_shapes) and fails if an
                                          instance x path is planned by none of them and is not shown unreachable;
  tests/test_epilogue_instances.py (GPU)  runs every problem below against the oracle and asserts that the expected instance ran.

Which instance a problem takes (lsx_plan.cpp, "launch shapes of the kernels around the sweep"), with L = 64 / Nrays wavelengths per tile,
nF the most fast continua of a tile, cells = 2 NLtot + Natoms if some tile's bound-free set is not simple, else 0, and
lk = min(most lines of a tile with linked continua, 4):
  LP   16 if L <= 16, 32 if L <= 32, else 64                                 (rays: 4 and more / 2, 3 / 1)
  NT   fixed(nt) = cells nt + 2 nF LP doubles; 256, halved to 128 and 64 while fixed(NT) > 3072
  SEG  Nspace (3 nF + 2 lk) + fixed(NT) > 5120
The topologies: one atom whose first continuum 0 -> 1 covers the whole spectrum and whose other continua -- 1 -> 2 (chained: a lower level
that is another continuum's upper level, so the set is not simple), 0 -> 2, then every pair of levels in turn -- cover the red half
only.  The blue tiles are simple, the red ones take the cells, so one launch runs both paths of its instance; the level count and
further atoms (one continuum each) set `cells`, the number of continua sets nF.  Seven, three and one ray: odd tile widths (9, 21) and
the full wave (64), none of which the column-mapped kernel takes.  Nothing here comes from the reference."""
from toy import spec_problem

PAIRS = [(0, 1), (1, 2), (0, 2)] + [(i, j) for j in range(3, 16) for i in range(j)]


def chain_atoms(nl0, k0, extra=(), nlk=0, red0=0.5):
    """atom 0 of nl0 levels: continuum 0 -> 1 everywhere, PAIRS[1 : k0] from `red0` on; nlk lines 0 -> nl0 - 1, 0 -> nl0 - 2 inside the
    red part, on levels no continuum ends on (the continua stay out of the sweep: linked); one more atom per entry of `extra` with that
    many levels and the continuum 0 -> top over the red part"""
    specs = [('l', 0, nl0 - 1 - u, red0 + 0.05 + 0.05 * u, 0.90 + 0.05 * u) for u in range(nlk)][::-1]
    specs += [('c',) + PAIRS[0] + (0.0, 1.0)] + [('c',) + PAIRS[q] + (red0, 1.0) for q in range(1, k0)]
    return [(nl0, specs)] + [(nl, [('c', 0, nl - 1, red0, 1.0)]) for nl in extra]


# a regular bound-free set under a line of its own atom that touches none of its upper levels (one linked line), on even tile widths:
# the column-mapped kernel by default, the row-mapped one with fast_rows=1
REGULAR = [(5, [('l', 0, 1, 0.30, 0.70), ('c', 0, 4, 0.00, 1.00), ('c', 2, 4, 0.00, 0.80), ('c', 3, 4, 0.20, 1.00)]),
           (3, [('c', 0, 2, 0.00, 0.60), ('c', 1, 2, 0.40, 1.00)])]

REGULAR_TWO = [(REGULAR[0][0], [('l', 0, 2, 0.35, 0.75)] + REGULAR[0][1]), REGULAR[1]]

SIMPLE_TWO = [(16, [('c', i, 15, 0.0, 1.0) for i in range(15)])] * 2

# name: (atoms, Nrays, Nspect, Nspace, options).  SEG cases: Nspace is the SMALLEST depth count at which the planner segments the column
# (tests/test_epilogue_ledger.py checks that one depth less is not segmented); the others: 9 to 40 depths, odd and even
CASES = {
    'r16_256':     (chain_atoms(5, 8), 7, 60, 21, None),
    'r16_256_seg': (chain_atoms(5, 8), 7, 60, 86, None),
    'r16_128':     (chain_atoms(8, 28), 7, 60, 24, None),
    'r16_128_seg': (chain_atoms(8, 28), 7, 60, 25, None),
    'r16_64':      (chain_atoms(13, 2, (10, 10)), 7, 60, 40, None),
    'r16_64_seg':  (chain_atoms(13, 2, (10, 10)), 7, 60, 49, None),
    'r32_256':     (chain_atoms(4, 6), 3, 70, 33, None),
    'r32_256_seg': (chain_atoms(4, 6), 2, 70, 136, None),
    'r32_128':     (chain_atoms(8, 14), 3, 70, 30, None),
    'r32_128_seg': (chain_atoms(8, 14), 2, 70, 49, None),
    'r32_64':      (chain_atoms(13, 2, (10, 10)), 2, 70, 27, None),
    'r32_64_seg':  (chain_atoms(13, 2, (10, 10)), 3, 70, 38, None),
    'r64_256':     (chain_atoms(4, 6, red0=0.7), 1, 100, 18, None),          # one ray: tiles of 64 and 36 wavelengths (nla < L)
    'r64_256_seg': (chain_atoms(4, 6, red0=0.7), 1, 100, 114, None),
    'r64_128':     (chain_atoms(6, 11, red0=0.7), 1, 100, 37, None),
    'r64_128_seg': (chain_atoms(6, 11, red0=0.7), 1, 100, 63, None),
    'r64_64':      (chain_atoms(13, 2, (10, 10), red0=0.7), 1, 100, 9, None),
    'r64_64_seg':  (chain_atoms(13, 2, (10, 10), red0=0.7), 1, 100, 17, None),
    # linked continua in row-mapped tiles, feeding one and two lines (the nLc rows of sL)
    'linked1':     (chain_atoms(5, 2, nlk=1), 7, 60, 23, None),
    'linked2':     (chain_atoms(6, 2, nlk=2), 3, 70, 32, None),
    # tiles the column-mapped kernel takes by default, through the row-mapped one
    'regular5':    (REGULAR, 5, 96, 29, 'fast_rows=1'),
    'regular4':    (REGULAR, 4, 90, 34, 'fast_rows=1'),
    # sixteen wavelengths per tile: with a linked line the column-mapped kernel's streams no longer fit its LDS, so the plan takes the
    # row-mapped kernel by itself -- simple tiles whose linked continua feed two lines, one of them ending on a continuum's lower level
    'regular4_two': (REGULAR_TWO, 4, 90, 35, None),
    'regular4_two_rows': (REGULAR_TWO, 4, 90, 36, 'fast_rows=1'),             # ... and its column-mapped tiles through it as well
    # no cells in the layout below 256 threads: two atoms of 16 levels, fifteen continua each onto the top level -- simple sets, 30
    # continua of two atoms in every tile (the per-atom grouping loop), 2 nF LP = 3840 > 3072 doubles at any thread count
    'simple64_64':     (SIMPLE_TWO, 1, 100, 14, None),
    'simple64_64_seg': (SIMPLE_TWO, 1, 100, 15, None),
}
NCOLS = (2, 33)          # the fused small-batch launch, one launch per tile class

# what each case plans (lsx_plan_epilogue_shapes; checked on the CPU against the plan, on the GPU against what ran): the row-mapped
# instance (LP, NT, SEG), its tiles on the simple path and on the cell path, the most lines its linked continua feed, the depths staged
# at a time, the tiles of the seven column-mapped lists, the tile classes with row-mapped tiles and with fast continua at all (each
# launches the row-mapped kernel / the pre-pass once per formal solution where every class has its own launches), whether the pre-pass
# stages the column in segments, the fewest wavelengths of a row-mapped tile (0: there is none).  'name:default': the same problem without the case's options
EXPECT = {
    'r16_256':      dict(rows=(16, 256, False), simple=3, cells=4, lk=0, seg_depths=21, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=6),
    'r16_256_seg':  dict(rows=(16, 256, True), simple=3, cells=4, lk=0, seg_depths=80, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=6),
    'r16_128':      dict(rows=(16, 128, False), simple=3, cells=4, lk=0, seg_depths=24, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=6),
    'r16_128_seg':  dict(rows=(16, 128, True), simple=3, cells=4, lk=0, seg_depths=24, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=6),
    'r16_64':       dict(rows=(16, 64, False), simple=3, cells=4, lk=0, seg_depths=40, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=6),
    'r16_64_seg':   dict(rows=(16, 64, True), simple=3, cells=4, lk=0, seg_depths=48, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=6),
    'r32_256':      dict(rows=(32, 256, False), simple=1, cells=3, lk=0, seg_depths=33, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=7),
    'r32_256_seg':  dict(rows=(32, 256, True), simple=1, cells=2, lk=0, seg_depths=128, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=6),
    'r32_128':      dict(rows=(32, 128, False), simple=1, cells=3, lk=0, seg_depths=30, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=7),
    'r32_128_seg':  dict(rows=(32, 128, True), simple=1, cells=2, lk=0, seg_depths=48, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=6),
    'r32_64':       dict(rows=(32, 64, False), simple=1, cells=2, lk=0, seg_depths=27, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=6),
    'r32_64_seg':   dict(rows=(32, 64, True), simple=1, cells=3, lk=0, seg_depths=36, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=7),
    'r64_256':      dict(rows=(64, 256, False), simple=1, cells=1, lk=0, seg_depths=18, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=36),
    'r64_256_seg':  dict(rows=(64, 256, True), simple=1, cells=1, lk=0, seg_depths=112, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=36),
    'r64_128':      dict(rows=(64, 128, False), simple=1, cells=1, lk=0, seg_depths=37, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=36),
    'r64_128_seg':  dict(rows=(64, 128, True), simple=1, cells=1, lk=0, seg_depths=62, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=36),
    'r64_64':       dict(rows=(64, 64, False), simple=1, cells=1, lk=0, seg_depths=9, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=36),
    'r64_64_seg':   dict(rows=(64, 64, True), simple=1, cells=1, lk=0, seg_depths=16, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=False, nla_min=36),
    'linked1':      dict(rows=(16, 256, False), simple=3, cells=4, lk=1, seg_depths=23, cols=(0, 0, 0, 0, 0, 0, 0), classes=(2, 2), prepass_seg=False, nla_min=6),
    'linked2':      dict(rows=(32, 128, False), simple=1, cells=3, lk=2, seg_depths=32, cols=(0, 0, 0, 0, 0, 0, 0), classes=(3, 3), prepass_seg=False, nla_min=7),
    'regular5:default': dict(rows=(16, 256, False), simple=0, cells=0, lk=0, seg_depths=29, cols=(4, 4, 0, 0, 0, 0, 0), classes=(0, 2), prepass_seg=False, nla_min=0),
    'regular5':     dict(rows=(16, 256, False), simple=8, cells=0, lk=1, seg_depths=29, cols=(0, 0, 0, 0, 0, 0, 0), classes=(2, 2), prepass_seg=False, nla_min=12),
    'regular4:default': dict(rows=(16, 256, False), simple=3, cells=0, lk=1, seg_depths=34, cols=(3, 0, 0, 0, 0, 0, 0), classes=(1, 2), prepass_seg=False, nla_min=16),
    'regular4':     dict(rows=(16, 256, False), simple=6, cells=0, lk=1, seg_depths=34, cols=(0, 0, 0, 0, 0, 0, 0), classes=(2, 2), prepass_seg=False, nla_min=10),
    'regular4_two': dict(rows=(16, 256, False), simple=4, cells=0, lk=2, seg_depths=35, cols=(2, 0, 0, 0, 0, 0, 0), classes=(2, 3), prepass_seg=False, nla_min=15),
    'regular4_two_rows:default': dict(rows=(16, 256, False), simple=4, cells=0, lk=2, seg_depths=36, cols=(2, 0, 0, 0, 0, 0, 0), classes=(2, 3), prepass_seg=False, nla_min=15),
    'regular4_two_rows': dict(rows=(16, 256, False), simple=6, cells=0, lk=2, seg_depths=36, cols=(0, 0, 0, 0, 0, 0, 0), classes=(3, 3), prepass_seg=False, nla_min=11),
    'simple64_64':  dict(rows=(64, 64, False), simple=2, cells=0, lk=0, seg_depths=14, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=True, nla_min=36),
    'simple64_64_seg': dict(rows=(64, 64, True), simple=2, cells=0, lk=0, seg_depths=14, cols=(0, 0, 0, 0, 0, 0, 0), classes=(1, 1), prepass_seg=True, nla_min=36),
}

# ledger rows no admissible problem plans, with the inequality of plan_build that shows why.  They stay in the product.
UNREACHABLE = {
    ('cols_list', 3): 'a tile is filed under a column-mapped list only if its linked continua feed at most two lines (lkn <= 2 in the '
                      'conditions of `cols` and `big`), and fgc_list() = lkclass() <= 2 (+ 4 for big sets) then: list 3 stays empty',
    ('finish_nt', 64): 'k_gamma_finish is chosen only if nl2max * 128 * 8 <= 48 KiB (the branch above sends everything else to '
                       'k_gamma_finish_levels), which is the negation of the halving loop\'s condition at finish_nt = 128',
    ('finish_nt', 32): 'as (finish_nt, 64): the loop that halves finish_nt cannot start',
}


def planned_rows(s):
    """ledger rows of a plan, from the vector of lsx_plan_epilogue_shapes"""
    rows = set()
    key = (s[0], s[1], bool(s[2]))
    if s[3] - s[4] > 0:
        rows.add(('rows',) + key + ('simple',))
    if s[4] > 0:
        rows.add(('rows',) + key + ('cells',))
    for v in range(7):
        if s[8 + v] > 0:
            rows.add(('cols', v, 6 if s[20] == 12 else 0) if v < 3 else (('cols_list', 3) if v == 3 else ('cols_big', v - 4)))
    if s[17] > 0:
        rows.add(('prepass', bool(s[15])))
    if s[18] == 0:
        rows.add(('finish_nt', s[19]))
    return rows


def expected_of(s):
    """the EXPECT entry a shapes vector amounts to"""
    return dict(rows=(s[0], s[1], bool(s[2])), simple=s[3] - s[4], cells=s[4], lk=s[21], seg_depths=s[6], cols=tuple(s[8:15]), classes=(s[24], s[25]), prepass_seg=bool(s[15]), nla_min=s[23])


def build(name, ncol, options_off=False):
    """-> (problem, columns, options).  tests/toy.py's collision rates and cross-sections as they are: the radiative part of every fast
    continuum's two Gamma entries is then no rounding-level addition to the collisional one (the CPU ledger asserts at least a tenth of
    the entry at half the depths or more; measured: at every depth of every case)"""
    atoms, Nrays, Nspect, Nspace, options = CASES[name]
    prob, block = spec_problem(atoms, seed=300 + list(CASES).index(name), Nspace=Nspace, Nrays=Nrays, Nspect=Nspect, ncol=ncol)
    return prob, block, (None if options_off else options)
