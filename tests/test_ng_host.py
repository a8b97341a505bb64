"""Ng acceleration of the MALI loop (include/lsx_hip_ng.h): what can be checked without a GPU.

The checker of the GPU tests is a numpy restatement of the scheme (tests/ng_cases.py).  It is pinned here by exactness -- Ng's
extrapolation of order m removes m geometric modes exactly -- and by the iteration counts the feature was specified with, over the
oracle; those runs are the recorded expectation of tests/test_ng.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ng_cases as ng
from conftest import ROOT
from lightspinner_amd import _capi
from lightspinner_amd.problem import Engine, NgOptions

CSRC = os.path.join(ROOT, 'lightspinner_amd', 'csrc')
U = ng.U


def geometric(rng, N, lams, amp=1e-2):
    """x_k = x* + sum_m v_m lam_m^k, k = len(lams) + 1 .. 0 -> (x*, [newest first])"""
    xstar = 10.0 ** rng.uniform(0.0, 6.0, N)
    modes = [amp * xstar * rng.uniform(0.5, 1.0, N) * rng.choice([-1.0, 1.0], N) for _ in lams]
    xs = [xstar + sum(v * lam ** k for v, lam in zip(modes, lams)) for k in range(len(lams) + 2)]
    return xstar, xs[::-1]


def exactness_bar(xs, order, c, A):
    """How far x_acc may be from x* when the x_k are a geometric sequence ROUNDED to float64.  Each x_k carries a relative error
    u, so in the weighted norm (w x^2 = 1) each column D_j of the least-squares problem min |d0 - sum c_j D_j|_w -- whose exact
    residual is zero -- moves by at most 4 u sqrt(N) (four terms) and d0 by 2 u sqrt(N): the minimiser moves by
    (|dD|_F |c|_2 + |dd0|) / sigma_min(D), sigma_min(D)^2 = lambda_min(A)  (Higham, Accuracy and Stability, Thm 20.1 with r = 0);
    forming and solving the normal equations adds (N + order) u cond(A) |c|_2 (tests/ng_cases.coefficients_bar).  Factor 2 for the
    second-order terms.  x_acc - x* = sum dc_j (x_j - x0) + the evaluation's own (order + 3) u (|1 - sum c| |x0| + sum |c_j| |x_j|)."""
    N = xs[0].size
    ev = np.linalg.eigvalsh(A)
    cond = ev[-1] / ev[0]
    cn = float(np.linalg.norm(c))
    dc = 2.0 * ((4 * U * np.sqrt(N * order) * cn + 2 * U * np.sqrt(N)) / np.sqrt(ev[0]) + (N + order) * U * cond * cn)
    spread = sum(np.abs(xs[j] - xs[0]) for j in range(1, order + 1))
    evalu = (order + 3) * U * (abs(1 - c.sum()) * np.abs(xs[0]) + sum(abs(cj) * np.abs(xs[j + 1]) for j, cj in enumerate(c)))
    return dc * spread + evalu, cond


@pytest.mark.parametrize('order,lams', [(1, (0.9,)), (1, (0.5,)), (2, (0.9, 0.5)), (2, (0.97, -0.6)), (2, (0.8, 0.7))])
@pytest.mark.parametrize('N', [6, 492])
def test_the_restatement_removes_as_many_geometric_modes_as_its_order(order, lams, N):
    rng = np.random.default_rng(100 * order + N)
    xstar, xs = geometric(rng, N, lams)
    c, xacc = ng.extrapolate(xs, order)
    A, _ = ng.normal_equations(xs, order)
    bar, cond = exactness_bar(xs, order, c, A)
    err = np.abs(xacc - xstar)
    print('order %d, lambda %s, N %d: cond(A) %.1e, |c| %.2f, error %.2e relative at worst, %.3f x the bar (bar %.1e relative)'
          % (order, lams, N, cond, np.abs(c).max(), (err / xstar).max(), (err / bar).max(), (bar / xstar).max()))
    assert (bar / xstar).max() < 1e-6, 'vacuous'
    assert np.all(err <= bar)
    # ... and it is an extrapolation: the newest iterate itself is ~1e-3 off
    assert (np.abs(xs[0] - xstar) / xstar).max() > 1e3 * (bar / xstar).max()


def test_one_order_too_few_does_not_remove_two_modes():
    """the exactness test can fail: order 1 on two modes leaves an error far above its bar"""
    rng = np.random.default_rng(7)
    xstar, xs = geometric(rng, 50, (0.9, 0.5))
    c, xacc = ng.extrapolate(xs[:3], 1)
    A, _ = ng.normal_equations(xs[:3], 1)
    bar, _ = exactness_bar(xs[:3], 1, c, A)
    assert np.any(np.abs(xacc - xstar) > 100 * bar)


def test_a_history_that_does_not_move_is_not_regular():
    x = np.full(10, 3.0)
    assert ng.extrapolate([x, x, x, x], 2) is None and ng.extrapolate([x, x, x], 1) is None


def test_the_state_machine_counts_as_specified():
    prob, _, _ = ng.problem('ca')
    col = ng.NgColumn(prob, 2, delay=2)
    rng = np.random.default_rng(3)
    xstar, xs = geometric(rng, prob.NLtot * prob.Nspace, (0.9, 0.5))
    seq = [x.reshape(prob.NLtot, prob.Nspace) for x in xs[::-1]]
    assert [col.stored] == [-2]
    assert col.after_stat_equil(seq[0]) is None and col.after_stat_equil(seq[0]) is None and col.stored == 0
    for k in range(3):
        assert col.after_stat_equil(seq[k]) is None and col.stored == k + 1
    out, dP = col.after_stat_equil(seq[3])
    assert col.stored == 0 and col.applied == 1 and col.rejected == 0 and col.hist == []
    assert dP == np.max(np.abs(1.0 - seq[2] / out))
    col.reset()
    assert col.stored == -2
    # a step that would go non-positive is rejected, and the history restarts all the same
    col = ng.NgColumn(prob, 1)
    a = np.full((prob.NLtot, prob.Nspace), 4.0)
    assert col.after_stat_equil(a) is None and col.after_stat_equil(0.5 * a) is None
    assert col.after_stat_equil(0.05 * a) is None and (col.applied, col.rejected, col.stored) == (0, 1, 0)


@pytest.mark.parametrize('case', ['ca', 'cah'])
def test_the_restatement_over_the_oracle_takes_the_specified_iterations(oracle_lib, case):
    plain, tight = ng.oracle_run(oracle_lib, case), ng.oracle_run(oracle_lib, case, tight=True)
    assert plain.converged and plain.n_iter == ng.PLAIN_ITERATIONS[case]
    assert tight.converged
    for order in (1, 2):
        r = ng.oracle_run(oracle_lib, case, order)
        print('%s order %d: %d iterations (plain %d), %d steps, %d rejected; off the 1e-8 plain run by %.2e (plain: %.2e)'
              % (case, order, r.n_iter, plain.n_iter, r.applied, r.rejected, ng.popdist(r.n, tight.n), ng.popdist(plain.n, tight.n)))
        assert r.converged and r.n_iter == ng.NG_ITERATIONS[case, order]
        assert r.rejected == 0 and r.applied >= 1
    assert ng.popdist(ng.oracle_run(oracle_lib, case, 2).n, tight.n) < ng.popdist(plain.n, tight.n)


def test_the_options_value_type():
    assert NgOptions() == NgOptions(2, 0) and NgOptions(1, 3) != NgOptions(1, 2) and repr(NgOptions(1, 3)) == 'NgOptions(order=1, delay=3)'
    assert len({NgOptions(2, 0), NgOptions(2, 0), NgOptions(1, 0)}) == 2
    for bad in ((3, 0), (-1, 0), (2, -1)):
        with pytest.raises(ValueError):
            NgOptions(*bad)


def test_the_oracle_has_no_such_entry_and_the_engine_says_so(oracle_lib):
    prob, block, _ = ng.problem('ca')
    e = Engine(prob, 1, lib=oracle_lib)
    assert not oracle_lib.has_ng
    with pytest.raises(NotImplementedError, match='lsx_hip_ng_configure'):
        e.configure_ng(2)
    with pytest.raises(NotImplementedError, match='lsx_hip_ng_state'):
        e.ng_state()
    e.close()


def test_the_entries_are_exported_and_declared_in_a_header_of_their_own():
    lib = os.path.join(CSRC, 'liblsx_hip.so')
    assert os.path.exists(lib), 'build the HIP library first (make -C lightspinner_amd/csrc)'
    syms = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
    text = open(os.path.join(ROOT, 'include', 'lsx_hip_ng.h')).read()
    declared = set(re.findall(r'\b(lsx_hip_[a-z0-9_]+)\s*\(', text))
    assert declared == {'lsx_hip_ng_configure', 'lsx_hip_ng_state'}
    assert set(re.findall(r'\bT (lsx_hip_ng[a-z0-9_]*)\b', syms)) == declared
    assert '#include "lsx_hip_ng.h"' in open(os.path.join(ROOT, 'include', 'lsx_hip.h')).read()
    assert not any(s.startswith('lsx_hip_ng') for s in _capi.REQUIRED_SYMBOLS)           # the common ABI is what it was
    assert 'lsx_hip_ng' not in open(os.path.join(ROOT, 'include', 'lsx.h')).read()
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    assert re.search(r'^BUILD_SRCS :=.*include/lsx_hip_ng\.h', mk, re.M)                   # part of the build id


@pytest.mark.parametrize('compiler,std', [('gcc', 'c99'), ('g++', 'c++11')])
def test_the_header_compiles_alone(compiler, std):
    lang = 'c' if compiler == 'gcc' else 'c++'
    r = subprocess.run([compiler, '-std=' + std, '-Wall', '-Wextra', '-pedantic', '-Werror', '-fsyntax-only', '-x', lang,
                        os.path.join(ROOT, 'include', 'lsx_hip_ng.h')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_kernels_use_no_scratch():
    """build/lsx_ng.ru.log, the compiler's resource report of the unit: every kernel without scratch, spilled VGPRs, dynamic stack"""
    path = os.path.join(CSRC, 'build', 'lsx_ng.ru.log')
    if not os.path.exists(path) and not os.path.exists(os.path.join(CSRC, 'liblsx_hip.so')) and shutil.which('hipcc') is None \
            and not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('nothing is built and there is no compiler')
    assert os.path.exists(path), 'build the HIP library first (make -C lightspinner_amd/csrc)'
    blocks = re.split(r'remark: [^\n]*Function Name: ', open(path).read())[1:]
    names = [b.split()[0] for b in blocks]
    assert len(names) == 3 and sum('k_ng_step' in x for x in names) == 2 and sum('k_ng_reset' in x for x in names) == 1, names
    for b in blocks:
        name = b.split()[0]
        val = lambda key: int(re.search(re.escape(key) + r':? (\d+)', b).group(1))
        assert val('ScratchSize [bytes/lane]') == 0, name
        assert val('VGPRs Spill') == 0, name
        assert re.search(r'Dynamic Stack: False', b), name
