"""The LTE-population kernel (lightspinner_amd/csrc/lsx_eqpops.hip) uses no scratch memory and no LDS: the compiler's per-kernel
resource report that the Makefile leaves beside the object (build/lsx_eqpops.ru.log) says ScratchSize 0, no spilled vector register,
no dynamic stack and 0 bytes of LDS -- the fields tests/test_no_scratch.py reads for the other units."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'lightspinner_amd', 'csrc')
LOG = os.path.join(CSRC, 'build', 'lsx_eqpops.ru.log')


def _report():
    if not os.path.exists(LOG):
        if shutil.which('hipcc') is None and not os.path.exists('/opt/rocm/bin/hipcc'):
            pytest.skip('no hipcc and no resource report')
        subprocess.check_call(['make', '-s', '-j', '8', '-C', CSRC])
    out = {}
    for blk in re.split(r'remark: Function Name: ', open(LOG).read())[1:]:
        get = lambda key: re.search(re.escape(key) + r': (\S+)', blk).group(1)
        out[blk.split()[0]] = dict(scratch=int(get('ScratchSize [bytes/lane]')), vspill=int(get('VGPRs Spill')), dynstack=get('Dynamic Stack'),
                                   lds=int(get('LDS Size [bytes/block]')))
    return out


def test_eq_pops_kernel_uses_no_scratch_and_no_lds():
    rep = _report()
    assert any('k_eq_pops' in name for name in rep), sorted(rep)
    bad = {k: v for k, v in rep.items() if v['scratch'] != 0 or v['vspill'] != 0 or v['dynstack'] != 'False' or v['lds'] != 0}
    assert not bad, bad
