"""The ctypes argument lists of the HIP-only entries (lightspinner_amd/_capi.py, HIP_FEATURES) against the prototypes of
include/lsx_hip*.h.  Tests and callers reach `lib.dll.lsx_hip_*` directly, so a wrong list is a silent ABI bug: every prototype is
translated to ctypes here and must be the table's list exactly."""
import ctypes as C
import glob
import os
import re

from conftest import ROOT
from lightspinner_amd import _capi

# declared for the tests' and the drivers' own use, bound where they are used: the only prototypes without a row in the table
NOT_BOUND = {'lsx_hip_request_hw_queues', 'lsx_hip_poison_lds'}

BY_VALUE = {'int32_t': C.c_int32, 'uint32_t': C.c_uint32, 'size_t': C.c_size_t, 'double': C.c_double, 'int': C.c_int}
POINTEE = {'double': C.c_double, 'int32_t': C.c_int32, 'int64_t': C.c_int64}
PROTOTYPE = re.compile(r'\b(int|int32_t)\s+(lsx_hip_\w+)\s*\(([^()]*)\)\s*;')


def struct_of(name):
    """lsx_fit_instrument -> _capi.LsxFitInstrument"""
    cls = getattr(_capi, ''.join(w.capitalize() for w in name.split('_')))
    assert issubclass(cls, C.Structure), name
    return cls


def to_ctypes(param):
    """one C parameter, name included -> its ctypes type"""
    words = param.replace('*', ' * ').replace('[', ' [').split()
    words = [w for w in words if w != 'const']
    array = words[-1].startswith('[')                       # double x[N]
    if array:
        words.pop()
    words.pop()                                             # the parameter's name
    base, stars = words[0], words.count('*') + (1 if array else 0)
    assert words == [base] + ['*'] * words.count('*') and stars <= 1, param
    if not stars:
        return BY_VALUE[base]
    if base == 'lsx_ctx':
        return C.c_void_p
    return C.POINTER(POINTEE[base] if base in POINTEE else struct_of(base))


def declared():
    """-> {symbol: (restype, [argtypes])} of every prototype in include/lsx_hip*.h"""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, 'include', 'lsx_hip*.h'))):
        with open(path) as f:
            text = f.read()
        text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
        text = re.sub(r'//[^\n]*', ' ', text)
        for ret, symbol, params in PROTOTYPE.findall(text):
            assert symbol not in out, symbol
            out[symbol] = (BY_VALUE[ret], [to_ctypes(p) for p in params.split(',')])
    return out


def bound():
    """-> {symbol: argtypes} of the table"""
    out = {}
    for feature, (phrase, entries) in _capi.HIP_FEATURES.items():
        assert phrase and entries, feature
        for symbol, argtypes in entries:
            assert symbol not in out, symbol
            out[symbol] = list(argtypes)
    return out


def test_the_translation_itself():
    assert to_ctypes('lsx_ctx* ctx') is C.c_void_p and to_ctypes('const lsx_ctx* ctx') is C.c_void_p
    assert to_ctypes('size_t nbytes') is C.c_size_t and to_ctypes('uint32_t parameters') is C.c_uint32
    assert to_ctypes('const double* mu') is to_ctypes('double *dst') is to_ctypes('double amp[4]') is C.POINTER(C.c_double)
    assert to_ctypes('const int32_t* ks') is C.POINTER(C.c_int32) and to_ctypes('int64_t* out') is C.POINTER(C.c_int64)
    assert to_ctypes('const lsx_fit_penalty* pen') is C.POINTER(_capi.LsxFitPenalty)


def test_every_prototype_is_bound_with_exactly_its_argument_list():
    have, want = bound(), declared()
    assert len(want) >= 42 and NOT_BOUND <= set(want)
    for symbol, (restype, argtypes) in sorted(want.items()):
        if symbol in NOT_BOUND:
            assert symbol not in have
            continue
        assert symbol in have, '%s is declared but has no row in _capi.HIP_FEATURES' % symbol
        assert have[symbol] == argtypes, symbol


def test_every_bound_symbol_is_declared():
    want = declared()
    assert sorted(set(bound()) - set(want)) == []
    assert len(bound()) == len(want) - len(NOT_BOUND)


def test_the_library_binds_the_table_in_its_order():
    """has_<feature> is the presence of the feature's FIRST entry; the names and the probes are those of every release so far"""
    probes = {f: entries[0][0] for f, (_, entries) in _capi.HIP_FEATURES.items()}
    assert probes == dict(
        emergent_rays='lsx_hip_emergent_rays', radiative_rates='lsx_hip_radiative_rates', radiative_losses='lsx_hip_radiative_losses',
        depth_rays='lsx_hip_depth_rays', spectrum='lsx_hip_spectrum', stokes='lsx_hip_stokes_rays', stokes_response='lsx_hip_response_stokes',
        fit_field='lsx_hip_fit_field_normal', fit_instrument='lsx_hip_instrument_fit_normal', stokes_velocity='lsx_hip_velocity_stokes_rays',
        fit_regular='lsx_hip_regular_penalty', background='lsx_hip_background', scales='lsx_hip_convert_scales', eq_pops='lsx_hip_eq_pops',
        ng='lsx_hip_ng_configure', time_dep='lsx_hip_time_dep_start', boundary='lsx_hip_set_boundary', epilogue_info='lsx_hip_epilogue_info')


class _Entry:
    argtypes = restype = None


class _Dll:
    """stands in for a ctypes.CDLL that exports `symbols`"""

    def __init__(self, symbols):
        for s in symbols:
            setattr(self, s, _Entry())


def test_binding_sets_argtypes_restype_and_the_flags():
    want = declared()
    lib = _capi.LsxLibrary.__new__(_capi.LsxLibrary)
    lib.dll = _Dll(bound())
    lib._bind_hip_features()
    for symbol, argtypes in bound().items():
        entry = getattr(lib.dll, symbol)
        assert entry.argtypes == argtypes and entry.restype is want[symbol][0], symbol
    assert all(getattr(lib, 'has_' + f) for f in _capi.HIP_FEATURES)
    none = _capi.LsxLibrary.__new__(_capi.LsxLibrary)
    none.dll = _Dll(())
    none._bind_hip_features()
    assert not any(getattr(none, 'has_' + f) for f in _capi.HIP_FEATURES)
