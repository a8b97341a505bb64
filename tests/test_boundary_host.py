"""The radiation boundary conditions without a GPU (include/lsx_hip_boundary.h): the fixture tests/golden/boundary_*.npz is well
posed, its generator's solver IS the reference's under the default kinds, the Python layer checks its arguments, and the setter's
host-side rules run under the sanitizers as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import boundary_cases as bc
import topology_cases as tc
import topology_reference as tr
from lightspinner_amd import boundary as B

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lightspinner_amd', 'csrc')


@pytest.mark.parametrize('name', bc.CASES)
def test_generator_solver_is_the_reference_under_the_default_kinds(name):
    """1: the generator ran its solver with (thermalised, zero) through the same loop and kept the SHA-256 of I, J and Gamma of both
    calls: the topology fixture, written by the reference's own piecewise_linear_1d, holds the same bits"""
    prob, block = tc.build(name)
    for col in tc.golden_columns(name, block.ncol):
        ref = tr.column_results(name, col)
        for k in bc.DEFAULT_KEYS:
            assert np.array_equal(bc.read('%s/%s/c%d/sha_%s' % (name, bc.DEFAULT, col, k)), bc.sha(ref[k])), (name, col, k)


@pytest.mark.parametrize('name', bc.CASES)
def test_fixture_is_well_posed(name):
    """2: computed from the inputs topology_cases.build gives; finite; and every stored combination moves Gamma of every call by at
    least 1e-3 of max |Gamma_default| -- what keeps a pass of the GPU test from meaning nothing"""
    prob, block = tc.build(name)
    cols = tc.golden_columns(name, block.ncol)
    for col in cols:
        assert np.array_equal(bc.read('%s/c%d/digest' % (name, col)), tc.input_digest(prob, block, col)), (name, col)
        dflt = tr.column_results(name, col)
        for combo in bc.COMBOS:
            for k in bc.KEYS:
                assert np.all(np.isfinite(bc.read('%s/%s/c%d/%s' % (name, combo, col, k)))), (name, combo, col, k)
            for call in (1, 2):
                G, G0 = bc.read('%s/%s/c%d/fs%d_Gamma' % (name, combo, col, call)), dflt['fs%d_Gamma' % call]
                assert G.shape == G0.shape
                moved = float(np.max(np.abs(G - G0)) / np.max(np.abs(G0)))
                assert moved >= 1e-3, (name, combo, col, call, moved)


class _Member:           # what an Enum member looks like to boundary.kind_code
    def __init__(self, name):
        self.name = name


def test_boundary_arguments():
    """3: kinds by string and by an enum-like object with .name; shapes; missing and superfluous arrays"""
    assert [B.kind_code(k) for k in ('zero', 'Thermalised', 'THERMALIZED', 'given', 0, 1, 2)] == [0, 1, 1, 2, 0, 1, 2]
    assert B.kind_code(_Member('Zero')) == B.ZERO and B.kind_code(_Member('Thermalised')) == B.THERMALISED
    for bad in ('reflecting', 3, -1, None, 1.0, True, _Member('Periodic')):
        with pytest.raises(ValueError):
            B.kind_code(bad)
    a = np.ones((7, 3))
    b = B.Boundary('given', _Member('Zero'), I_lower=a)
    assert (b.lower, b.upper) == (B.GIVEN, B.ZERO) and b.I_upper is None and b.I_lower.flags['C_CONTIGUOUS'] and not b.is_default
    assert B.Boundary().is_default and B.Boundary('thermalised', 'zero').is_default
    with pytest.raises(ValueError, match='I_lower is needed'):
        B.Boundary('given', 'zero')
    with pytest.raises(ValueError, match='I_upper is needed'):
        B.Boundary('zero', 'given', I_upper=None)
    with pytest.raises(ValueError, match='I_upper was handed over'):
        B.Boundary('given', 'zero', I_lower=a, I_upper=a)
    with pytest.raises(ValueError, match='I_lower was handed over'):
        B.Boundary('thermalised', 'zero', I_lower=a)
    with pytest.raises(ValueError, match='expected \\[Nspect\\]\\[Nrays\\]'):
        B.Boundary('given', 'zero', I_lower=np.ones(7))
    with pytest.raises(ValueError, match='differ in shape'):
        B.Boundary('given', 'given', I_lower=a, I_upper=np.ones((7, 4)))

    class Atmos:
        lowerBc, upperBc = _Member('Zero'), _Member('Thermalised')
    f = B.Boundary.from_atmos(Atmos())
    assert (f.lower, f.upper) == (B.ZERO, B.THERMALISED)
    # the engine's own check of the arrays against its shape
    assert B._array(a, B.GIVEN, 'lower', (7, 3), 4).shape == (4, 7, 3)          # one column's array for every column
    assert B._array(np.ones((4, 7, 3)), B.GIVEN, 'lower', (7, 3), 4).shape == (4, 7, 3)
    with pytest.raises(ValueError, match='expected \\(4, 7, 3\\)'):
        B._array(np.ones((3, 7, 3)), B.GIVEN, 'lower', (7, 3), 4)


def test_engine_on_the_oracle_refuses(oracle_lib):
    """the entry is the HIP library's alone: a clear error on an engine bound to the oracle"""
    from lightspinner_amd.problem import Engine
    prob, block = tc.build('toy-see7-Nra8-Nsp21-Nsp48-nco2')
    e = Engine(prob, block.ncol, lib=oracle_lib)
    with pytest.raises(NotImplementedError, match='lsx_hip_set_boundary'):
        e.set_boundary('zero', 'zero')
    with pytest.raises(NotImplementedError, match='lsx_hip_boundary_state'):
        e.boundary_state()
    e.close()


def test_context_boundary_none_makes_no_call(oracle_lib, monkeypatch):
    """3: rh_method.Context(boundary=None) -- the drop-in's default -- never reaches the setter; 'atmos' and a Boundary do, with the
    kinds they carry; anything else is refused"""
    from helpers import build_fakes
    from conftest import golden
    from lightspinner_amd.problem import Engine
    from lightspinner_amd.rh_method import Context
    calls = []
    monkeypatch.setattr(Engine, 'set_boundary', lambda self, *a, **kw: calls.append((a, kw)))
    d = dict(np.load(golden('falc_ca.npz')))

    def make(**kw):
        atmos, spect, eq, bg = build_fakes(d)
        atmos.lowerBc, atmos.upperBc = _Member('Zero'), _Member('Thermalised')      # the reference ignores them: so does None
        return Context(atmos, spect, eq, bg, lib=oracle_lib, **kw)
    make().close()
    make(boundary=None).close()
    assert calls == []
    make(boundary='atmos').close()
    assert len(calls) == 1 and (calls[0][0][0].lower, calls[0][0][0].upper) == (B.ZERO, B.THERMALISED)
    given = B.Boundary('zero', 'zero')
    make(boundary=given).close()
    assert len(calls) == 2 and calls[1][0][0] is given
    for bad in ('zero', 3, ('zero', 'zero')):
        with pytest.raises(ValueError, match='boundary must be'):
            make(boundary=bad)


def test_setter_rules_under_asan_ubsan():
    """4: the host-side rules of lsx_hip_set_boundary (lsx_boundary_prep.h) as a stand-alone program under
    -fsanitize=address,undefined (`make bndsan`); nothing is loaded into python"""
    subprocess.check_call(['make', '-s', '-C', CSRC, 'bndsan'])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    out = subprocess.run([os.path.join(CSRC, 'lsx_bnd_san')], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and out.stdout.strip() == 'ok', (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
