"""Ledger of the compiled instances of the fast-continuum epilogue (CPU side; the GPU side is tests/test_epilogue_instances.py, the shared
data tests/epilogue_cases.py): an instance that lsx_plan.h lists is compiled into the product and can be dispatched to, so some GPU
parity test has to plan it -- on each of the row-mapped kernel's two paths -- or the planner's arithmetic has to exclude it.  The plans
and launch shapes come from the product's own planner (lsx_plan.cpp built into liblsx_host.so, `make host`), not from a restatement."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden
import epilogue_cases as ec
from lightspinner_amd import _capi, fixtures
from lightspinner_amd.problem import Problem, Transition

CSRC = os.path.join(ROOT, 'lightspinner_amd', 'csrc')
pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='no host compiler')
FALC = ('falc_ca.npz', 'falc_cah.npz', 'falc_c.npz', 'falc_fe.npz', 'falc_mg.npz', 'falc_all.npz')


@pytest.fixture(scope='module')
def host():
    subprocess.check_call(['make', '-s', '-C', CSRC, 'host'])
    from san_driver import HostOnly
    h = HostOnly(os.path.join(CSRC, 'liblsx_host.so'))
    h.dll.lsx_plan_epilogue_instances.restype = C.c_int32
    h.dll.lsx_plan_epilogue_instances.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.c_int32]
    h.dll.lsx_plan_epilogue_shapes.argtypes = [C.POINTER(_capi.LsxProblem), C.c_uint32, C.POINTER(C.c_int64), C.c_char_p, C.c_int32]
    return h


def _shapes_c(host, p, bits=0):
    out = (C.c_int64 * 26)()
    err = C.create_string_buffer(512)
    rc = host.dll.lsx_plan_epilogue_shapes(C.byref(p), bits, out, err, 512)
    return (rc, err.value.decode(), [int(x) for x in out])


def shapes(host, prob, bits=0):
    p, keep = prob.to_c()
    rc, msg, s = _shapes_c(host, p, bits)
    assert rc == 0, msg
    return s


def compiled(host):
    """every ledger row the product compiles: the row-mapped instances on both of their paths, the column-mapped ones, the pre-pass"""
    def codes(which):
        buf = (C.c_int32 * 64)()
        n = host.dll.lsx_plan_epilogue_instances(which, buf, 64)
        assert 0 < n <= 64
        return [int(buf[i]) for i in range(n)]
    rows = [(c >> 10, (c & 1023) >> 1, bool(c & 1)) for c in codes(0)]
    assert len(rows) == len(set(rows)) == 18
    out = [('rows',) + r + (path,) for r in rows for path in ('simple', 'cells')]
    out += [('cols', c >> 4, c & 15) for c in codes(1)] + [('cols_big', c) for c in codes(2)] + [('prepass', bool(c)) for c in codes(3)]
    assert len(out) == 36 + 6 + 3 + 2
    return out


def _bits(options):
    assert options in (None, 'fast_rows=1')
    return 8 if options else 0


def planned_by_gpu_tests(host):
    """{ledger row: [who plans it]} over the cases of tests/epilogue_cases.py and the problems of the existing GPU parity modules"""
    import instance_cases as ic
    from toy import toy_problem
    from test_toy_topologies import CASES as TOY, RS_CASES
    who = {}

    def note(name, prob, bits=0):
        for r in ec.planned_rows(shapes(host, prob, bits)):
            who.setdefault(r, []).append(name)
    for name in ec.CASES:
        prob, _, options = ec.build(name, 1)
        note('epilogue_cases:' + name, prob, _bits(options))
        if options:
            note('epilogue_cases:' + name + ':default', prob)
    for kw in TOY + RS_CASES:                                       # tests/test_toy_topologies.py
        note('toy:seed%d' % kw['seed'], toy_problem(**dict(kw, ncol=1))[0])
    for name, ncol, Ns, compact in ic.CASES:                        # tests/test_instances_gpu.py
        note('instance_cases:' + name, ic.build(name, 1, Ns, compact)[0])
    for fx in FALC:                                                 # tests/test_production_classes.py, tests/test_hip_parity.py
        note(fx, fixtures.load_problem_npz(golden(fx), phi_compact=False)[0])
    return who


def check_ledger(host):
    who = planned_by_gpu_tests(host)
    rows = compiled(host)
    orphans = [r for r in rows if r not in who and r not in ec.UNREACHABLE]
    assert orphans == [], 'compiled epilogue instances that no GPU parity test plans and nothing shows unreachable: %s' % orphans
    assert [r for r in ec.UNREACHABLE if r in who] == []
    # nothing is planned that has no instance (a launch switch without a matching instance launches nothing)
    extra = [r for r in who if r not in rows and r[0] != 'finish_nt']
    assert extra == [], extra
    return who


def test_every_compiled_instance_is_planned_or_shown_unreachable(host):
    who = check_ledger(host)
    # the row-mapped instances are this module's own: each of the 36 (instance, path) rows by a case of tests/epilogue_cases.py
    for r in compiled(host):
        if r[0] == 'rows':
            assert any(w.startswith('epilogue_cases:') for w in who[r]), (r, who[r])


def test_the_ledger_names_an_instance_whose_case_is_removed(host, monkeypatch):
    """negative control: without its case the ledger fails and says which instance lost its test"""
    monkeypatch.delitem(ec.CASES, 'r32_64_seg')
    with pytest.raises(AssertionError, match=r"\('rows', 32, 64, True, 'simple'\), \('rows', 32, 64, True, 'cells'\)"):
        check_ledger(host)


def test_each_case_plans_what_the_table_says(host):
    assert set(ec.EXPECT) == set(ec.CASES) | {n + ':default' for n, c in ec.CASES.items() if c[4]}
    for name, (atoms, Nrays, Nspect, Nspace, options) in ec.CASES.items():
        prob, _, _ = ec.build(name, 1)
        s = shapes(host, prob, _bits(options))
        assert ec.expected_of(s) == ec.EXPECT[name], (name, ec.expected_of(s))
        if options:
            assert ec.expected_of(shapes(host, prob)) == ec.EXPECT[name + ':default'], name
        assert Nspect <= 100
        if ec.EXPECT[name]['rows'][2]:
            # the smallest depth count at which the planner segments this column, and more than one segment's worth of depths
            prob.Nspace = Nspace - 1
            assert not shapes(host, prob, _bits(options))[2], name
            assert ec.EXPECT[name]['seg_depths'] < Nspace
        else:
            assert 9 <= Nspace <= 40 and ec.EXPECT[name]['seg_depths'] == Nspace, name
        if Nrays == 1:
            assert 0 < s[23] < 64 and ec.EXPECT[name]['nla_min'] == s[23], name      # a ragged last tile (nla < L) under LP = 64
    # a problem whose tiles go to the column-mapped kernel by default also runs them through the row-mapped one
    for name, c in ec.CASES.items():
        if not c[4] and any(ec.EXPECT[name]['cols']):
            assert any(d[0] is c[0] and d[1] == c[1] and d[4] == 'fast_rows=1' for d in ec.CASES.values()), name
    # odd and even depth counts, a ragged last tile under 64 lanes per row, linked continua feeding one and two lines on both paths
    assert {c[3] % 2 for c in ec.CASES.values() if c[3] <= 40} == {0, 1}
    # the simple path below 256 threads with the cells in front of the staged operands, and without them
    assert any(e['rows'][1] < 256 and e['simple'] and e['cells'] for e in ec.EXPECT.values())
    assert {e['rows'] for e in ec.EXPECT.values() if e['rows'][1] < 256 and e['simple'] and not e['cells']} == {(64, 64, False), (64, 64, True)}
    lk = {(e['lk'], e['simple'] > 0 and e['cells'] == 0) for e in ec.EXPECT.values()}
    assert {(1, True), (2, True), (1, False), (2, False)} <= lk


def _grid_problem(Nrays, nlev, k, Nspace):
    """one atom of nlev levels whose first k level pairs are bound-free continua over the whole spectrum: k fast continua per tile"""
    L = 64 // Nrays
    Nspect = L + 3
    wavelength = 100.0 + np.arange(Nspect, dtype=np.float64)
    x, w = np.polynomial.legendre.leggauss(Nrays)
    trans = [Transition(0, False, i, j, 0, Nspect, lambda0=float(wavelength[-1]), alpha=np.full(Nspect, 1e-22)) for i, j in ec.PAIRS[:k]]
    return Problem(Nspace=Nspace, wavelength=wavelength, muz=0.5 * x + 0.5, wmu=0.5 * w, Nlevel=[nlev], trans=trans,
                   active=np.ones((k, Nspect), dtype=np.uint8))


def test_nothing_unreachable_is_planned(host):
    """400 random transition tables, a grid over ray counts, level counts, fast continua per tile and depths, the reference's problems:
    no plan has a row of UNREACHABLE, and every row-mapped shape that is planned has an instance"""
    from san_driver import random_problem
    rows = set(compiled(host))
    seen = set()

    def check(s):
        got = ec.planned_rows(s)
        bad = [r for r in got if r in ec.UNREACHABLE or (r not in rows and r[0] != 'finish_nt')]
        assert bad == [], bad
        seen.update(got)
    rng = np.random.default_rng(2024)
    for _ in range(400):
        p, keep = random_problem(rng).to_c()
        for bits in (0, 8, 32, 1):                                  # default, fast_rows, finish_lds, LSX_NO_LINKED
            rc, msg, s = _shapes_c(host, p, bits)
            if rc != 0:
                assert rc in (1, 5), msg
                continue
            check(s)
    for fx in FALC:
        prob = fixtures.load_problem_npz(golden(fx), phi_compact=False)[0]
        for bits in (0, 8, 32):
            check(shapes(host, prob, bits))
    n = 0
    for Nrays in (1, 2, 3, 4, 5, 7, 8, 16):
        for nlev in range(2, 17):
            for k in range(1, min(48, nlev * (nlev - 1) // 2) + 1):
                p, keep = _grid_problem(Nrays, nlev, k, 3).to_c()
                for Nspace in (3, 40, 200, 1500):
                    p.Nspace = Nspace
                    for bits in (0, 32):
                        rc, msg, s = _shapes_c(host, p, bits)
                        if rc != 0:
                            assert rc == 5, msg                     # LSX_EUNSUPPORTED: an LDS request above 64 KiB
                            continue
                        check(s)
                        n += 1
    assert n > 20000
    # the survey is no empty one: all 18 row-mapped shapes, both pre-pass instances and k_gamma_finish at 128 threads occur in it
    assert len({r[1:4] for r in seen if r[0] == 'rows'}) == 18 and {('prepass', False), ('prepass', True), ('finish_nt', 128)} <= seen


def test_the_cases_are_not_vacuous(host, oracle_lib):
    """on the oracle, every case: the radiative part of Gamma (Gamma minus the collisional matrix) is at least a tenth of the entry at
    half the depths or more, for both entries of every fast continuum -- a wrong epilogue cannot hide under the collisions"""
    from lightspinner_amd.problem import Engine
    for name in ec.CASES:
        prob, block, _ = ec.build(name, 2)
        e = Engine(prob, 2, lib=oracle_lib)
        e.set_columns(0, block)
        e.formal_sol_gamma()
        G = e.get(_capi.LSX_GAMMA)
        e.close()
        for t in prob.trans:
            if t.is_line:
                continue
            nl, o = prob.Nlevel[t.atom], prob.lev2_off[t.atom]
            for a, b in ((t.i, t.j), (t.j, t.i)):
                g, c = G[:, o + a * nl + b, :], block.C[:, o + a * nl + b, :]
                share = (np.abs(g - c) >= 0.1 * np.abs(g)).mean(axis=1)
                assert share.min() >= 0.5, (name, t.atom, a, b, share)
