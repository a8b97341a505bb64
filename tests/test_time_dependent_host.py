"""The implicit rate-equation step without a GPU (include/lsx_hip_timedep.h): the solve of lsx_solve_dev.h compiled for the CPU
(liblsx_td_host.so) on the inputs of the GPU tests -- every family, size and shape, Gamma from the oracle's formal solution --
against the exact solve and its bars (tests/td_cases.py), which also verifies the redraw cap and the vacuity assertion before
anything goes to a GPU; the stand-alone sanitizer program; header, binding and export; the resource report; and the checker's
own pins."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import td_cases as td
from conftest import ROOT
from lightspinner_amd import _capi

ENTRIES = ('lsx_hip_time_dep_start', 'lsx_hip_time_dep_update_async', 'lsx_hip_time_dep_update', 'lsx_hip_time_dep_state')


@pytest.fixture(scope='module')
def host():
    return td.HostLib()


@pytest.mark.parametrize('Nl', td.NLS)
@pytest.mark.parametrize('name', sorted(td.FAMILIES))
def test_host_family(oracle_lib, host, name, Nl):
    """the register form up to 8 levels, the in-memory form above; the in-memory form gives the register form's bits"""
    res = {}
    td.family(td.HostRunner(oracle_lib, host), name, Nl, results=res)
    if Nl <= 8 and name == 'rate_scale':
        mem = {}
        td.family(td.HostRunner(oracle_lib, host, in_memory=True), name, Nl, results=mem)
        for key in res:
            assert np.array_equal(res[key][2].view(np.uint64), mem[key][2].view(np.uint64)), key


def test_formulas_under_asan_ubsan():
    """325 systems of every size 2 ... 16 in both forms, a frozen column, a singular and a NaN system, the refusals: in a
    stand-alone program"""
    subprocess.check_call(['make', '-s', '-C', td.CSRC, 'tdsan'])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    out = subprocess.run([os.path.join(td.CSRC, 'lsx_td_san')], capture_output=True, text=True, timeout=600, env=env)
    tail = out.stdout[-1500:] + '\n' + out.stderr[-3000:]
    assert out.returncode == 0, tail
    assert 'TIMEDEP SANITIZED RUN COMPLETE' in out.stdout, tail


def test_header_binding_and_export_agree():
    hdr = open(os.path.join(ROOT, 'include', 'lsx_hip_timedep.h')).read()
    declared = re.findall(r'^int (lsx_hip_\w+)\(([^;]*)\);', hdr, flags=re.M)
    assert tuple(n for n, _ in declared) == ENTRIES
    assert '#include "lsx_hip_timedep.h"' in open(os.path.join(ROOT, 'include', 'lsx_hip.h')).read()
    path = _capi.hip_library_path()
    if not os.path.exists(path):
        pytest.fail('the HIP library is not built: %s' % path)
    dll = C.CDLL(path)           # (loading the library needs no device)
    kinds = {'lsx_ctx*': C.c_void_p, 'int32_t': C.c_int32, 'const double*': C.POINTER(C.c_double), 'double*': C.POINTER(C.c_double)}
    lib = _capi.LsxLibrary(path)
    assert lib.has_time_dep
    for name, args in declared:
        assert hasattr(dll, name), name
        want = [kinds[re.sub(r'\s*\w+$', '', a.strip())] for a in args.split(',')]
        fn = getattr(lib.dll, name)
        assert list(fn.argtypes) == want, name
        assert fn.restype is C.c_int


def test_the_oracle_does_not_have_the_entries(oracle_lib):
    from lightspinner_amd.problem import Engine
    assert not oracle_lib.has_time_dep
    prob, block, _ = td.probe_problem([2], 7, 3)
    e = Engine(prob, 3, lib=oracle_lib)
    for call in (lambda: e.time_dep_start(1.0), e.time_dep_update, e.time_dep_update_async, e.time_dep_state):
        with pytest.raises(NotImplementedError):
            call()
    e.close()


def test_the_kernels_use_no_scratch_and_spill_no_vector_register():
    log = os.path.join(td.CSRC, 'build', 'lsx_timedep.ru.log')
    if not os.path.exists(log):
        if shutil.which('hipcc') is None and not os.path.exists('/opt/rocm/bin/hipcc'):
            pytest.skip('no hipcc and no resource report')
        subprocess.check_call(['make', '-s', '-j', '8', '-C', td.CSRC])
    rep = {}
    for blk in re.split(r'remark: Function Name: ', open(log).read())[1:]:
        get = lambda key: re.search(re.escape(key) + r': (\S+)', blk).group(1)
        rep[blk.split()[0]] = dict(scratch=int(get('ScratchSize [bytes/lane]')), vspill=int(get('VGPRs Spill')), dynstack=get('Dynamic Stack'))
    reg = [n for n in rep if 'k_time_dep_reg' in n]
    assert len(reg) == 7 and sum('k_time_dep' in n for n in rep) == 8, sorted(rep)
    bad = {k: v for k, v in rep.items() if v['scratch'] != 0 or v['vspill'] != 0 or v['dynstack'] != 'False'}
    assert not bad, bad


def test_checker_against_the_closed_form_of_two_levels():
    td.closed_form_two_levels()


def test_checker_with_the_wrong_right_hand_side_misses_its_bar(oracle_lib, host):
    td.wrong_variant_misses_its_bar(td.HostRunner(oracle_lib, host))


def test_driver_runs_on_a_scripted_engine():
    """advance_time_columns' own logic -- the call sequence, freezing, the counts, max_iter, the all_done hook -- on a scripted engine"""
    from lightspinner_amd import drivers

    class Scripted:
        ncol = 3

        def __init__(self):
            self.calls, self.mask, self.it = [], None, 0

        def set_active_columns(self, m):
            self.mask = None if m is None else np.array(m, dtype=bool)
            self.calls.append(('mask', None if m is None else tuple(bool(x) for x in m)))

        def time_dep_start(self, dt):
            self.calls.append(('start', dt))
            self.it = 0

        def formal_sol_gamma(self):
            self.it += 1
            self.calls.append(('fs',))

        def time_dep_update(self):
            self.calls.append(('td',))

        def get(self, what):
            # column c needs c + 2 iterations; column 2 never gets there
            need = np.array([2, 3, 99])
            v = np.where(self.it >= need, 1e-6, 1.0)
            if what == _capi.LSX_DPOPS_COL and self.mask is not None:
                v = np.where(self.mask, v, 0.0)
            return v

    e = Scripted()
    asked = []
    counts = drivers.advance_time_columns(e, 0.5, nsteps=2, max_iter=6, all_done=lambda d: asked.append(d) or d)
    assert counts.tolist() == [[2, 3, 6], [2, 3, 6]]
    assert [c for c in e.calls if c[0] == 'start'] == [('start', 0.5)] * 2
    assert e.calls[0] == ('mask', None) and e.calls[-1] == ('mask', None)
    assert ('mask', (False, True, True)) in e.calls and ('mask', (False, False, True)) in e.calls
    assert asked == [False] * 5 + [True] + [False] * 5 + [True]
    assert sum(c == ('fs',) for c in e.calls) == 12 == sum(c == ('td',) for c in e.calls)
