"""The background kernels (lightspinner_amd/csrc/lsx_background.hip) use no scratch memory: the compiler's per-kernel resource report
that the Makefile leaves beside the object (build/lsx_background.ru.log) says ScratchSize 0, no spilled vector register and no
dynamic stack for every kernel of the unit -- the same three fields tests/test_no_scratch.py reads for the other units.  Fe I's
48-term sum and the table lookups index constant tables, never a runtime-indexed private array."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'lightspinner_amd', 'csrc')
LOG = os.path.join(CSRC, 'build', 'lsx_background.ru.log')


def _report():
    if not os.path.exists(LOG):
        if shutil.which('hipcc') is None and not os.path.exists('/opt/rocm/bin/hipcc'):
            pytest.skip('no hipcc and no resource report')
        subprocess.check_call(['make', '-s', '-j', '8', '-C', CSRC])
    out = {}
    for blk in re.split(r'remark: Function Name: ', open(LOG).read())[1:]:
        get = lambda key: re.search(re.escape(key) + r': (\S+)', blk).group(1)
        out[blk.split()[0]] = dict(scratch=int(get('ScratchSize [bytes/lane]')), vspill=int(get('VGPRs Spill')), dynstack=get('Dynamic Stack'))
    return out


def test_background_kernels_use_no_scratch():
    rep = _report()
    for kernel in ('k_eos', 'k_bg_wave', 'k_background_opacity', 'k_bg_sca'):
        assert any(kernel in name for name in rep), (kernel, sorted(rep))
    bad = {k: v for k, v in rep.items() if v['scratch'] != 0 or v['vspill'] != 0 or v['dynstack'] != 'False'}
    assert not bad, bad
