"""What every HIP-only Engine method hands to the library, pinned without a library: a recording stand-in takes the place of
lightspinner_amd._capi.LsxLibrary.  Its `dll` attributes note (symbol, arguments) and return 0, so that the sequence of entries a
call reaches, the number of arguments, every by-value argument (ranges and windows resolved, byte counts) and which pointers are
NULL can be compared with what include/lsx_hip*.h asks for.  The numbers themselves are the GPU suite's business."""
import os

import numpy as np
import pytest

from conftest import ROOT
from lightspinner_amd import boundary, fit, fixtures
from lightspinner_amd.problem import DepthRays, Engine, RadiativeLosses

P = 'ptr'            # a pointer argument that is not NULL (an array, a struct by reference, the handle)
FEATURES = ('emergent_rays', 'radiative_rates', 'radiative_losses', 'depth_rays', 'spectrum', 'stokes', 'stokes_response', 'fit_field',
            'fit_instrument', 'stokes_velocity', 'fit_regular', 'background', 'scales', 'eq_pops', 'ng', 'time_dep', 'boundary',
            'epilogue_info')


class _Dll:
    def __init__(self, calls):
        self._calls = calls

    def __getattr__(self, symbol):
        def entry(*args):
            self._calls.append((symbol, args))
            return 49 if symbol == 'lsx_hip_epilogue_info' else 0          # (the length of its counter list: include/lsx_hip_epilogue.h)
        return entry


class RecordingLibrary:
    path, backend = '/nowhere/librecording.so', 'recording'

    def __init__(self, have=FEATURES):
        self.calls = []
        self.dll = _Dll(self.calls)
        for f in FEATURES:
            setattr(self, 'has_' + f, f in have)

    def check(self, rc):
        assert rc == 0

    def take(self):
        """-> [(symbol, [per argument: its value if passed by value, None if NULL, P otherwise])] since the last take()"""
        out = []
        for symbol, args in self.calls:
            seen = []
            for a in args:
                if isinstance(a, (bool, np.bool_)):
                    raise AssertionError('%s: a bool among the arguments' % symbol)
                seen.append(None if a is None else int(a) if isinstance(a, (int, np.integer)) else
                            float(a) if isinstance(a, (float, np.floating)) else P)
            out.append((symbol, seen))
        del self.calls[:]
        return out


class Untouchable:
    """an argument that may not be looked at"""

    def _no(self, *a, **k):
        raise AssertionError('an argument was read before the missing feature was reported')
    __array__ = __int__ = __float__ = __index__ = __iter__ = __len__ = __bool__ = __getattr__ = _no


class Tables:
    """what Engine wants of a background.EosTables"""

    def to_c(self):
        from lightspinner_amd import _capi
        return _capi.LsxEosTables(), None


class Levels:
    E_SI, g, stage = [0.0, 1e-18], [2.0, 1.0], [0, 1]


@pytest.fixture(scope='module')
def prob():
    return fixtures.load_problem_npz(os.path.join(ROOT, 'tests', 'golden', 'falc_ca.npz'))[0]


@pytest.fixture
def eng(prob):
    lib = RecordingLibrary()
    e = Engine(prob, 2, lib=lib)
    assert [s for s, _ in lib.take()] == ['lsx_create_with_options']
    return e


MUS, LA0, NMU = [1.0, 0.5], 3, 2
FIELD = (0.1, 0.2, 0.3)


def stokes_prefix(prob):
    """handle, angles, columns [1, 2), wavelengths [3, Nspect), three fields, four pattern arrays"""
    return [P, NMU, P, 1, 1, LA0, prob.Nspect - LA0, P, P, P, P, P, P, P]


def test_emergent_rays(eng, prob):
    eng.emergent_rays(MUS, col0=1)
    assert eng.lib.take() == [('lsx_hip_emergent_rays', [P, 2, P, 1, 1, P, prob.Nspect * 2 * 8])]
    eng.emergent_rays(1.0, col0=0, ncol=2)
    assert eng.lib.take() == [('lsx_hip_emergent_rays', [P, 1, P, 0, 2, P, 2 * prob.Nspect * 8])]


def test_emergent_spectrum(eng, prob):
    ncont, Ns = prob.Ntrans - prob.Nlines, prob.Nspace
    eng.emergent_spectrum([1.0], [500.0, 501.0, 502.0], alpha=np.zeros((ncont, 3)), col0=1, work_cap_bytes=1 << 20)
    assert eng.lib.take() == [('lsx_hip_spectrum_work_cap', [P, 1 << 20]),
                              ('lsx_hip_spectrum', [P, 3, P, P, None, None, None, 1, P, 1, 1, P, 3 * 8])]
    eng.emergent_spectrum(MUS, [500.0, 501.0], bg_chi=np.zeros((2, 2, Ns)), bg_eta=np.zeros((2, 2, Ns)))
    assert eng.lib.take() == [('lsx_hip_spectrum', [P, 2, P, None, P, P, None, 2, P, 0, 2, P, 2 * 2 * 2 * 8])]


def test_radiative_rates(eng, prob):
    eng.radiative_rates(col0=1, work_cap_bytes=0)
    assert eng.lib.take() == [('lsx_hip_radiative_rates_work_cap', [P, 0]),
                              ('lsx_hip_radiative_rates', [P, 1, 1, P, P, P, prob.Ntrans * prob.Nspace * 8])]
    eng.radiative_rates()
    assert eng.lib.take() == [('lsx_hip_radiative_rates', [P, 0, 2, P, P, P, 2 * prob.Ntrans * prob.Nspace * 8])]


def test_radiative_losses_and_frequency_weights(eng, prob):
    Ns, Nt, Nsp = prob.Nspace, prob.Ntrans, prob.Nspect
    eng.frequency_weights()
    assert eng.lib.take() == [('lsx_hip_frequency_weights', [Nsp, P, P])]
    eng.radiative_losses(col0=1, what=('F', 'Qt'), work_cap_bytes=4096)
    want = [P if w in ('F', 'Qt') else None for w in RadiativeLosses.FIELDS]
    assert eng.lib.take() == [('lsx_hip_radiative_losses_work_cap', [P, 4096]),
                              ('lsx_hip_frequency_weights', [Nsp, P, P]),
                              ('lsx_hip_radiative_losses', [P, 1, 1, None] + want + [Ns * 8, Nt * Ns * 8, Nsp * Ns * 8])]
    eng.radiative_losses(wnu=np.ones(Nsp), what='Q')
    want = [P if w == 'Q' else None for w in RadiativeLosses.FIELDS]
    assert eng.lib.take() == [('lsx_hip_radiative_losses', [P, 0, 2, P] + want + [2 * Ns * 8, 2 * Nt * Ns * 8, 2 * Nsp * Ns * 8])]


def test_depth_rays(eng, prob):
    Ns, nla = prob.Nspace, prob.Nspect - LA0
    eng.depth_rays([1.0], la0=LA0, col0=1, what=('tau', 'z_tau1'), work_cap_bytes=1 << 16)
    want = [P if w in ('tau', 'z_tau1') else None for w in DepthRays.FIELDS]
    assert eng.lib.take() == [('lsx_hip_depth_rays_work_cap', [P, 1 << 16]),
                              ('lsx_hip_depth_rays', [P, 1, P, 1, 1, LA0, nla] + want + [Ns * nla * 8, nla * 8])]
    eng.depth_rays(MUS, la0=2, nla=5)
    assert eng.lib.take() == [('lsx_hip_depth_rays', [P, 2, P, 0, 2, 2, 5] + [P] * 6 + [2 * 2 * Ns * 5 * 8, 2 * 2 * 5 * 8])]


def test_stokes_rays_without_a_velocity(eng, prob):
    eng.stokes_rays(MUS, *FIELD, la0=LA0, col0=1, work_cap_bytes=1 << 20)
    assert eng.lib.take() == [('lsx_hip_stokes_rays_work_cap', [P, 1 << 20]),
                              ('lsx_hip_stokes_rays', stokes_prefix(prob) + [P, 4 * (prob.Nspect - LA0) * NMU * 8])]


def test_stokes_rays_with_a_velocity(eng, prob):
    eng.stokes_rays(MUS, *FIELD, la0=LA0, col0=1, vlos=10.0)
    assert eng.lib.take() == [('lsx_hip_velocity_stokes_rays', stokes_prefix(prob) + [P, 4 * (prob.Nspect - LA0) * NMU * 8, P])]
    eng.stokes_rays([1.0], np.zeros((2, prob.Nspace)), 0.0, 0.0, la0=1, nla=4, vlos=np.zeros(prob.Nspace))
    assert eng.lib.take() == [('lsx_hip_velocity_stokes_rays', [P, 1, P, 0, 2, 1, 4] + [P] * 7 + [P, 2 * 4 * 4 * 8, P])]


def response_tail(prob, bits, nparam, nk, ks_given):
    nla = prob.Nspect - LA0
    return [bits, P, nk, P if ks_given else None, P, nparam * 4 * nla * nk * NMU * 8, P, 4 * nla * NMU * 8]


def test_stokes_response_without_a_velocity(eng, prob):
    eng.stokes_response(MUS, *FIELD, la0=LA0, col0=1, parameters=('chiB', 'B'), ks=[0, 5], work_cap_bytes=1 << 20)
    assert eng.lib.take() == [('lsx_hip_response_stokes_work_cap', [P, 1 << 20]),
                              ('lsx_hip_response_stokes', stokes_prefix(prob) + response_tail(prob, 5, 2, 2, True))]
    eng.stokes_response(MUS, *FIELD, la0=LA0, col0=1)
    assert eng.lib.take() == [('lsx_hip_response_stokes', stokes_prefix(prob) + response_tail(prob, 7, 3, prob.Nspace, False))]


def test_stokes_response_with_a_velocity_or_its_response(eng, prob):
    eng.stokes_response(MUS, *FIELD, la0=LA0, col0=1, parameters=('vlos', 'gammaB'), ks=[4])           # velocity zero
    assert eng.lib.take() == [('lsx_hip_velocity_response_stokes', stokes_prefix(prob) + response_tail(prob, 10, 2, 1, True) + [P])]
    eng.stokes_response(MUS, *FIELD, la0=LA0, col0=1, vlos=10.0)
    assert eng.lib.take() == [('lsx_hip_velocity_response_stokes',
                               stokes_prefix(prob) + response_tail(prob, 7, 3, prob.Nspace, False) + [P])]
    eng.stokes_response(MUS, *FIELD, la0=LA0, col0=1, vlos=10.0, parameters='vlos', work_cap_bytes=0)
    assert eng.lib.take() == [('lsx_hip_response_stokes_work_cap', [P, 0]),
                              ('lsx_hip_velocity_response_stokes',
                               stokes_prefix(prob) + response_tail(prob, 8, 1, prob.Nspace, False) + [P])]


def fit_case(prob, nq, instrument, weight=False, base=False):
    """-> (positional arguments, keywords, the 15 arguments of the entries' head)"""
    Ns, nla = prob.Nspace, prob.Nspect - LA0
    nnode = (1, 1, 0, 2)[:nq] if nq == 4 else (1, 1, 0)
    npar = int(sum(nnode))
    inst = fit.Instrument(np.arange(0, nla - 1, 2), np.ones(((nla - 1 + 1) // 2, 2)), nla) if instrument else None
    nobs = inst.nobs if instrument else nla
    kw = dict(la0=LA0, col0=1, instrument=inst)
    if weight:
        kw['weight'] = 2.0
    if base:
        kw['base'] = np.zeros((nq, Ns))
    head = [P, NMU, P, 1, 1, LA0, nla, P, P, P, P, P, P, P if base else None, P]
    return (MUS, np.ones((npar, Ns)), nnode, np.zeros(npar), np.zeros((1, 4, nobs, NMU))), kw, head


FIT_ENTRY = {(3, False): 'lsx_hip_fit_field_%s', (3, True): 'lsx_hip_instrument_fit_%s', (4, False): 'lsx_hip_velocity_fit_%s',
             (4, True): 'lsx_hip_velocity_fit_%s'}


@pytest.mark.parametrize('nq,instrument', sorted(FIT_ENTRY))
def test_fit_field_normal(eng, prob, nq, instrument):
    args, kw, head = fit_case(prob, nq, instrument, weight=instrument, base=(nq == 4))
    eng.fit_field_normal(*args, work_cap_bytes=1 << 22, **kw)
    inst = [] if (nq, instrument) == (3, False) else [P if instrument else None]
    assert eng.lib.take() == [('lsx_hip_fit_field_work_cap', [P, 1 << 22]),
                              (FIT_ENTRY[nq, instrument] % 'normal', head + [P, P, P if instrument else None, P, P, P, P] + inst)]


@pytest.mark.parametrize('nq,instrument', sorted(FIT_ENTRY))
def test_fit_field_chi2(eng, prob, nq, instrument):
    args, kw, head = fit_case(prob, nq, instrument, weight=not instrument, base=(nq == 3))
    eng.fit_field_chi2(*args, **kw)
    inst = [] if (nq, instrument) == (3, False) else [P if instrument else None]
    assert eng.lib.take() == [(FIT_ENTRY[nq, instrument] % 'chi2', head + [P, None if instrument else P, P, P] + inst)]


def test_fit_field_step(eng):
    eng.fit_field_step(np.eye(2)[None], np.ones((1, 2)), 0.1, np.zeros(2))
    assert eng.lib.take() == [('lsx_hip_fit_field_step', [P, 1, 2] + [P] * 9)]
    eng.fit_field_step(np.stack([np.eye(3)] * 2), np.ones((2, 3)), [0.1, 0.2], np.zeros((2, 3)), lo=-1.0, hi=np.ones(3))
    assert eng.lib.take() == [('lsx_hip_fit_field_step', [P, 2, 3] + [P] * 9)]


def test_fit_field_penalty(eng):
    pen = fit.Penalty(np.eye(2), target=[1.0, 2.0])
    eng.fit_field_penalty(np.zeros((1, 2)), pen, [1.0])
    assert eng.lib.take() == [('lsx_hip_regular_penalty', [P, 1, 2, P, P, P, None, None, P])]
    eng.fit_field_penalty(np.zeros((3, 2)), pen, np.ones(3), grad=np.zeros((3, 2)), hess=np.zeros((3, 2, 2)))
    assert eng.lib.take() == [('lsx_hip_regular_penalty', [P, 3, 2, P, P, P, P, P, P])]


def test_fit_field_uncertainty(eng, prob):
    Ns = prob.Nspace
    eng.fit_field_uncertainty(np.eye(2), np.ones((2, Ns)), (1, 1, 0))
    assert eng.lib.take() == [('lsx_hip_regular_uncertainty', [P, 1, 2, P, None, None, 3, P, P, Ns, P, P, P, P, P])]
    eng.fit_field_uncertainty(np.stack([np.eye(2)] * 2), np.ones((2, 7)), (1, 0, 0, 1), penalty=fit.Penalty(np.eye(2)), scale=2.0,
                              ainv=False, field_sigma=False)
    assert eng.lib.take() == [('lsx_hip_regular_uncertainty', [P, 2, 2, P, P, P, 4, P, P, 7, None, P, P, None, P])]


def test_apply_instrument(eng):
    eng.apply_instrument(np.zeros((3, 4, 6, 2)), fit.Instrument.identity(6))
    assert eng.lib.take() == [('lsx_hip_instrument_apply', [P, P, 6, 2, 12, P, P])]


def test_eos_and_background(eng, prob):
    Ns, Nsp = prob.Nspace, prob.Nspect
    T = np.full(Ns, 5000.0)
    eng.eos(Tables(), T, T)
    assert eng.lib.take() == [('lsx_hip_eos', [P, P, 1] + [P] * 6)]
    eng.background(Tables(), np.stack([T] * 2), np.stack([T] * 2), np.stack([T] * 2))
    assert eng.lib.take() == [('lsx_hip_background', [P, P, 0, 2, P, P, P, Nsp, None, P, P, P, 0])]
    eng.background(Tables(), T, T, T, col0=1, install=True, read_back=False)
    assert eng.lib.take() == [('lsx_hip_background', [P, P, 1, 1, P, P, P, Nsp, None, None, None, None, 1])]
    eng.background(Tables(), T, T, T, wavelength=[400.0, 500.0])
    assert eng.lib.take() == [('lsx_hip_background', [P, P, 0, 1, P, P, P, 2, P, P, P, P, 0])]


def test_convert_scales(eng, prob):
    from lightspinner_amd import _capi
    T = np.full(prob.Nspace, 5000.0)
    eng.convert_scales(Tables(), 'tau500', T, T, T, col0=1)
    assert eng.lib.take() == [('lsx_hip_convert_scales', [P, P, _capi.LSX_SCALE_TAU500, 1, 1, P, P, P, None, 10**2.44, P, P, P, P, 0])]
    eng.convert_scales(Tables(), 'geometric', T, T, T, ne=T, logG=2.0, install=True, read_back=False)
    assert eng.lib.take() == [('lsx_hip_convert_scales', [P, P, _capi.LSX_SCALE_GEOMETRIC, 0, 1, P, P, P, P, 100.0] + [None] * 4 + [1])]


def test_eq_pops(eng, prob):
    T = np.full((2, prob.Nspace), 5000.0)
    eng.eq_pops([Levels(), Levels()], [1.0, 1e-4], T, T, T)
    assert eng.lib.take() == [('lsx_hip_eq_pops', [P, 2, P, 2, P, P, P, P, P])]
    eng.eq_pops([Levels()], [1.0], T[0], T[0], T[0], want_nTotal=False)
    assert eng.lib.take() == [('lsx_hip_eq_pops', [P, 1, P, 1, P, P, P, P, None])]


def test_ng(eng):
    eng.configure_ng(2, 3)
    eng.configure_ng(None)
    eng.ng_state(col0=1)
    assert eng.lib.take() == [('lsx_hip_ng_configure', [P, 2, 3]), ('lsx_hip_ng_configure', [P, 0, 0]),
                              ('lsx_hip_ng_state', [P, 1, 1, P, P, P, P])]


def test_boundary(eng, prob):
    eng.set_boundary('zero', 'zero', col0=1)
    eng.set_boundary('given', 'thermalised', I_lower=np.zeros((prob.Nspect, prob.Nrays)))
    eng.boundary_state(col0=1)
    assert eng.lib.take() == [('lsx_hip_set_boundary', [P, 1, 1, boundary.ZERO, boundary.ZERO, None, None]),
                              ('lsx_hip_set_boundary', [P, 0, 2, boundary.GIVEN, boundary.THERMALISED, P, None]),
                              ('lsx_hip_boundary_state', [P, 1, 1, P])]


def test_time_dependent(eng, prob):
    eng.time_dep_start(0.5, col0=1)
    eng.time_dep_start([0.5, 0.25], n_prev=np.zeros((2, prob.NLtot, prob.Nspace)))
    eng.time_dep_update()
    eng.time_dep_update_async()
    eng.time_dep_state(col0=1)
    assert eng.lib.take() == [('lsx_hip_time_dep_start', [P, 1, 1, P, None]), ('lsx_hip_time_dep_start', [P, 0, 2, P, P]),
                              ('lsx_hip_time_dep_update', [P, P]), ('lsx_hip_time_dep_update_async', [P]),
                              ('lsx_hip_time_dep_state', [P, 1, 1, P, P])]


def test_epilogue_info(eng):
    info = eng.epilogue_info()
    assert eng.lib.take() == [('lsx_hip_epilogue_info', [P, P])]
    assert info['rows'] == {} and info['cols'] == [0] * 7


# ---- a library without the feature: reported by the entry's C name, before an argument is looked at ----
X = Untouchable()
GUARD_FIRST = [          # (the entry named, the call, with arguments that may not be read)
    ('lsx_hip_epilogue_info', lambda e: e.epilogue_info()),
    ('lsx_hip_emergent_rays', lambda e: e.emergent_rays(X, col0=X, ncol=X)),
    ('lsx_hip_spectrum', lambda e: e.emergent_spectrum(X, X, alpha=X, col0=X, ncol=X, work_cap_bytes=X)),
    ('lsx_hip_radiative_rates', lambda e: e.radiative_rates(col0=X, ncol=X, work_cap_bytes=X)),
    ('lsx_hip_frequency_weights', lambda e: e.frequency_weights()),
    ('lsx_hip_radiative_losses', lambda e: e.radiative_losses(col0=X, ncol=X, wnu=X, what=X, work_cap_bytes=X)),
    ('lsx_hip_depth_rays', lambda e: e.depth_rays(X, la0=X, nla=X, col0=X, ncol=X, what=X, work_cap_bytes=X)),
    ('lsx_hip_stokes_rays', lambda e: e.stokes_rays(X, X, X, X, patterns=X, la0=X, nla=X, col0=X, ncol=X, work_cap_bytes=X, vlos=X)),
    ('lsx_hip_response_stokes', lambda e: e.stokes_response(X, X, X, X, patterns=X, la0=X, nla=X, col0=X, ncol=X, parameters=X,
                                                            amplitudes=X, ks=X, work_cap_bytes=X, vlos=X)),
    ('lsx_hip_fit_field_normal', lambda e: e.fit_field_normal(X, X, X, X, X, weight=X, base=X, patterns=X, la0=X, nla=X, col0=X, ncol=X,
                                                              amplitudes=X, work_cap_bytes=X, instrument=X)),
    ('lsx_hip_fit_field_chi2', lambda e: e.fit_field_chi2(X, X, X, X, X, weight=X, base=X, patterns=X, la0=X, nla=X, col0=X, ncol=X,
                                                          work_cap_bytes=X, instrument=X)),
    ('lsx_hip_fit_field_step', lambda e: e.fit_field_step(X, X, X, X, lo=X, hi=X)),
    ('lsx_hip_eos', lambda e: e.eos(X, X, X)),
    ('lsx_hip_background', lambda e: e.background(X, X, X, X, wavelength=X, col0=X, install=X, read_back=X)),
    ('lsx_hip_convert_scales', lambda e: e.convert_scales(X, X, X, X, X, ne=X, logG=X, col0=X, install=X, read_back=X)),
    ('lsx_hip_eq_pops', lambda e: e.eq_pops(X, X, X, X, X, want_nTotal=X)),
    ('lsx_hip_ng_configure', lambda e: e.configure_ng(X, X)),
    ('lsx_hip_ng_state', lambda e: e.ng_state(col0=X, ncol=X)),
    ('lsx_hip_set_boundary', lambda e: e.set_boundary(X, X, I_lower=X, I_upper=X, col0=X, ncol=X)),
    ('lsx_hip_boundary_state', lambda e: e.boundary_state(col0=X, ncol=X)),
    ('lsx_hip_time_dep_start', lambda e: e.time_dep_start(X, n_prev=X, col0=X, ncol=X)),
    ('lsx_hip_time_dep_update', lambda e: e.time_dep_update()),
    ('lsx_hip_time_dep_update_async', lambda e: e.time_dep_update_async()),
    ('lsx_hip_time_dep_state', lambda e: e.time_dep_state(col0=X, ncol=X)),
]
# these three look at the shapes of their arrays first, as they always did: the feature is asked for where the struct is made
SHAPES_FIRST = [
    ('lsx_hip_instrument_fit_normal', lambda e: e.apply_instrument(np.zeros((4, 6, 2)), fit.Instrument.identity(6))),
    ('lsx_hip_regular_penalty', lambda e: e.fit_field_penalty(np.zeros((1, 2)), fit.Penalty(np.eye(2)), [1.0])),
    ('lsx_hip_regular_uncertainty', lambda e: e.fit_field_uncertainty(np.eye(2), np.ones((2, 5)), (1, 1, 0))),
    ('lsx_hip_regular_penalty', lambda e: e.fit_field_uncertainty(np.eye(2), np.ones((2, 5)), (1, 1, 0), penalty=fit.Penalty(np.eye(2)))),
]


@pytest.mark.parametrize('entry,call', GUARD_FIRST + SHAPES_FIRST, ids=[c[0] + '-%d' % i for i, c in enumerate(GUARD_FIRST + SHAPES_FIRST)])
def test_a_library_without_the_features_is_reported_by_the_entry(prob, entry, call):
    lib = RecordingLibrary(have=())
    e = Engine(prob, 2, lib=lib)
    lib.take()
    with pytest.raises(NotImplementedError, match=r'%s\b' % entry) as err:
        call(e)
    assert lib.path in str(err.value) and '(%s)' % lib.backend in str(err.value)
    assert lib.take() == []


def test_a_library_object_without_the_attributes_counts_as_one_without_the_features(prob):
    lib = RecordingLibrary()
    for f in FEATURES:
        delattr(lib, 'has_' + f)
    e = Engine(prob, 1, lib=lib)
    with pytest.raises(NotImplementedError, match='lsx_hip_stokes_rays'):
        e.stokes_rays([1.0], *FIELD)
    with pytest.raises(NotImplementedError, match='lsx_hip_time_dep_update_async'):
        e.time_dep_update_async()


@pytest.mark.parametrize('which', ['normal', 'chi2'])
def test_the_later_features_are_asked_for_where_a_call_needs_them(prob, which):
    """a library with the Stokes pass and the fit, but without the velocity of a call or the instrument"""
    lib = RecordingLibrary(have=('stokes', 'stokes_response', 'fit_field'))
    e = Engine(prob, 2, lib=lib)
    with pytest.raises(NotImplementedError, match='lsx_hip_velocity_stokes_rays'):
        e.stokes_rays(MUS, *FIELD, vlos=1.0)
    with pytest.raises(NotImplementedError, match='lsx_hip_velocity_response_stokes'):
        e.stokes_response(MUS, *FIELD, parameters='vlos')
    call = getattr(e, 'fit_field_' + which)
    args, kw, _ = fit_case(prob, 4, False)
    with pytest.raises(NotImplementedError, match='lsx_hip_velocity_fit_' + which):
        call(*args, **kw)
    args, kw, _ = fit_case(prob, 3, True)
    with pytest.raises(NotImplementedError, match='lsx_hip_instrument_fit_normal'):
        call(*args, **kw)
    assert 'lsx_hip_fit_field_' + which not in [s for s, _ in lib.take()]
    args, kw, head = fit_case(prob, 3, False)
    call(*args, **kw)
    assert lib.take()[-1][0] == 'lsx_hip_fit_field_' + which
