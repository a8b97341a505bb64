"""The statistical-equilibrium solve, system by system, at every size (tests/se_cases.py): on the oracle here, on the HIP library
under -m gpu -- the register instances k_stat_equil_reg<2..8>, the LDS kernel from 9 to 16 levels, the refusal at 17 -- and, here
again, the device's own solve (lsx_solve_dev.h) compiled for the CPU on the oracle's Gamma."""
import pytest

import se_cases
import td_cases
from se_cases import NLS

FAMILIES = sorted(se_cases.FAMILIES)


@pytest.mark.parametrize('Nl', NLS)
@pytest.mark.parametrize('name', FAMILIES)
def test_oracle_family(oracle_lib, name, Nl):
    se_cases.family(oracle_lib, name, Nl)


def test_oracle_two_probe_atoms(oracle_lib):
    se_cases.two_probe_atoms(oracle_lib)


def test_oracle_gamma_of_a_probe_atom_is_its_rates(oracle_lib):
    se_cases.gamma_is_the_rates(oracle_lib)


@pytest.mark.parametrize('calls', ['sync', 'async'])
def test_oracle_one_singular_system_among_regular_ones(oracle_lib, calls):
    se_cases.one_singular_system(oracle_lib, calls)


def test_oracle_names_the_system_the_reference_raises_on_first(oracle_lib):
    se_cases.first_singular_system(oracle_lib)


@pytest.mark.parametrize('Nl', [2, 5, 9])
def test_oracle_nan_in_the_rates_is_a_singular_system(oracle_lib, Nl):
    se_cases.nan_in_the_rates(oracle_lib, Nl)


# ---- the device's solve, compiled for the CPU ---------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host():
    return td_cases.HostLib()


@pytest.mark.parametrize('Nl', NLS)
@pytest.mark.parametrize('name', FAMILIES)
def test_host_family(oracle_lib, host, name, Nl):
    """the register form up to 8 levels (the in-memory form at work strides 1 and 64 gives its bits), the in-memory form above"""
    se_cases.host_family(oracle_lib, host, name, Nl)


@pytest.mark.parametrize('Nl', [5, 9])
def test_host_singular_and_nan_systems_among_regular_ones(oracle_lib, host, Nl):
    se_cases.host_bad_systems(oracle_lib, host, Nl)


# ---- the HIP library ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def both():
    """the new populations of the families on both libraries, for the reported hip-to-oracle difference"""
    return {}, {}


@pytest.mark.gpu
@pytest.mark.parametrize('Nl', NLS)
@pytest.mark.parametrize('name', FAMILIES)
def test_hip_family(hip_lib, oracle_lib, both, name, Nl):
    se_cases.family(hip_lib, name, Nl, results=both[0])
    se_cases.family(oracle_lib, name, Nl, results=both[1], check=False)
    se_cases.hip_against_oracle({k: v for k, v in both[0].items() if k[:2] == (name, Nl)}, both[1])


@pytest.mark.gpu
def test_hip_two_probe_atoms(hip_lib):
    se_cases.two_probe_atoms(hip_lib)


@pytest.mark.gpu
@pytest.mark.parametrize('options', [None, 'finish_big=0', 'finish_big=1', 'finish_big=1,finish_lds=1'])
def test_hip_gamma_of_a_probe_atom_is_its_rates(hip_lib, options):
    se_cases.gamma_is_the_rates(hip_lib, options)


@pytest.mark.gpu
@pytest.mark.parametrize('Nl', [5, 9])
@pytest.mark.parametrize('calls', ['sync', 'async'])
def test_hip_one_singular_system_among_regular_ones(hip_lib, calls, Nl):
    se_cases.one_singular_system(hip_lib, calls, Nl)


@pytest.mark.gpu
def test_hip_names_the_system_the_reference_raises_on_first(hip_lib):
    se_cases.first_singular_system(hip_lib)


@pytest.mark.gpu
@pytest.mark.parametrize('Nl', [2, 5, 9])
def test_hip_nan_in_the_rates_is_a_singular_system(hip_lib, Nl):
    se_cases.nan_in_the_rates(hip_lib, Nl)


@pytest.mark.gpu
def test_hip_refuses_seventeen_levels_when_the_context_is_made(hip_lib):
    se_cases.too_many_levels(hip_lib)


@pytest.mark.gpu
@pytest.mark.parametrize('Nl', range(2, 9))
def test_hip_register_and_lds_instances_give_the_same_bits(hip_lib, Nl):
    se_cases.instances_agree(hip_lib, Nl)
