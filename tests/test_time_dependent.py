"""Time-dependent populations on the GPU (include/lsx_hip_timedep.h; Engine.time_dep_*, Context.time_dep_update,
drivers.advance_time_columns): the implicit rate-equation step system by system against the exact solve and its bars
(tests/td_cases.py, whose checker and inputs tests/test_time_dependent_host.py runs on the CPU), the protocol around it, and the
driver."""
import pytest

import td_cases as td

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('Nl', td.NLS)
@pytest.mark.parametrize('name', sorted(td.FAMILIES))
def test_family(hip_lib, name, Nl):
    """1, 4: every system against the exact solve, LSX_DPOPS_COL, number conservation; blocking and enqueued give the same bits"""
    td.family(td.HipRunner(hip_lib), name, Nl, calls=('sync', 'async'))


@pytest.mark.parametrize('Nl', [2, 3, 4, 5, 6, 7, 8])
def test_register_and_lds_instances_agree(hip_lib, Nl):
    td.instances_agree(hip_lib, Nl)


@pytest.mark.parametrize('Nl', [2, 5, 8, 9, 16])
def test_limits_of_long_and_short_steps(hip_lib, Nl):
    td.limits(hip_lib, Nl)


@pytest.mark.parametrize('Nl', [3, 8, 12])
def test_second_update_from_another_iterate(hip_lib, Nl):
    td.second_update_from_another_iterate(hip_lib, Nl)


def test_frozen_columns(hip_lib):
    td.frozen_columns(hip_lib)


@pytest.mark.parametrize('Nl', [5, 9])
@pytest.mark.parametrize('calls', ['sync', 'async'])
def test_one_nan_rate_among_regular_systems(hip_lib, calls, Nl):
    td.one_bad_system(hip_lib, calls, Nl)


def test_refusals_change_nothing(hip_lib):
    td.refusals(hip_lib)


def test_state_returns_what_start_was_given(hip_lib):
    td.state_round_trip(hip_lib)


def test_ng_history_is_discarded_and_the_options_never_change(hip_lib):
    td.ng_history_and_options(hip_lib)


def test_a_columns_bits_do_not_depend_on_the_context(hip_lib):
    td.sharding(hip_lib)


def test_driver_against_the_closed_form(hip_lib):
    td.driver_closed_form(hip_lib)


@pytest.mark.parametrize('which', ['toy', 'falc_ca'])
def test_driver_with_radiation(hip_lib, which):
    td.driver_with_radiation(hip_lib, which)


@pytest.mark.parametrize('lookahead', [True, False])
def test_context_time_dep_update(hip_lib, lookahead):
    td.context_time_dep_update(hip_lib, lookahead)
