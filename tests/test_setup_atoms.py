"""The set-up chain on all five of the reference's model atoms and at its edges (tests/setup_cases.py): on the oracle here,
on the HIP library under -m gpu, where it is compared with the reference's values and with the oracle's."""
import pytest

import setup_cases


def test_oracle_five_atoms_against_the_reference(oracle_lib):
    setup_cases.five_atoms_against_the_reference(oracle_lib)


def test_oracle_collision_spline_against_scipy(oracle_lib):
    setup_cases.collision_spline_against_scipy(oracle_lib)


def test_oracle_refuses_tables_it_cannot_interpolate(oracle_lib):
    setup_cases.spline_refusals(oracle_lib)


@pytest.mark.gpu
def test_hip_five_atoms_against_the_reference_and_the_oracle(hip_lib, oracle_lib):
    eh, _ = setup_cases.five_atoms_against_the_reference(hip_lib)
    eo, _ = setup_cases.five_atoms_against_the_reference(oracle_lib)
    setup_cases.against_each_other(eh, eo, 'hip vs oracle, five atoms')


@pytest.mark.gpu
def test_hip_collision_spline_against_scipy_and_the_oracle(hip_lib, oracle_lib):
    h = setup_cases.collision_spline_against_scipy(hip_lib)
    o = setup_cases.collision_spline_against_scipy(oracle_lib)
    setup_cases.outputs_against_each_other(h, o, 'hip vs oracle, spline')


@pytest.mark.gpu
def test_hip_refuses_tables_it_cannot_interpolate(hip_lib):
    setup_cases.spline_refusals(hip_lib)


@pytest.mark.parametrize('with_vlos', [False, True])
def test_oracle_voigt_across_the_a_v_plane(oracle_lib, with_vlos):
    setup_cases.voigt_plane(oracle_lib, with_vlos)


@pytest.mark.gpu
@pytest.mark.parametrize('with_vlos', [False, True])
def test_hip_voigt_across_the_a_v_plane(hip_lib, oracle_lib, with_vlos):
    h = setup_cases.voigt_plane(hip_lib, with_vlos)
    o = setup_cases.voigt_plane(oracle_lib, with_vlos)
    setup_cases.outputs_against_each_other(h, o, 'hip vs oracle, voigt')
