"""Flat, column-batched description of the hot-path inputs and the Engine that
feeds them through the lsx C ABI.

`Problem`      -- what is common to every column: grids, quadrature, transition table
                  (what rh_method.Context.__init__ derives from `spect`, rh_method.py:531-563)
`ColumnBlock`  -- per-column arrays with a leading [ncol] index, in the reference's
                  own layouts (rh_method.py:387-423 and 93-131)
`Engine`       -- owns one lsx_ctx (one device, one stream)
"""
import ctypes as C
import itertools
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _capi
from ._capi import f64, _ptr, _iptr, _opt


def _vector(a):
    """a scalar or any array (viewing angles, wavelengths) -> float64 [n]"""
    return f64(np.atleast_1d(np.asarray(a, dtype=np.float64)).reshape(-1))


@dataclass
class Transition:
    atom: int
    is_line: bool
    i: int
    j: int
    Nblue: int
    Nlambda: int
    Aji: float = 0.0
    Bji: float = 0.0
    Bij: float = 0.0
    lambda0: float = 0.0
    alpha: Optional[np.ndarray] = None  # continua: [Nlambda]


@dataclass
class Problem:
    Nspace: int
    wavelength: np.ndarray          # [Nspect] nm
    muz: np.ndarray                 # [Nrays]
    wmu: np.ndarray                 # [Nrays]
    Nlevel: List[int]               # per active atom
    trans: List[Transition]         # ordered as [t for atom in activeAtoms for t in atom.trans]
    active: np.ndarray              # bool [Ntrans][Nspect]
    sca_per_lambda: bool = False
    phi_compact: bool = False
    atom_names: List[str] = field(default_factory=list)

    def __post_init__(self):
        self.wavelength = f64(self.wavelength)
        self.muz = f64(self.muz)
        self.wmu = f64(self.wmu)
        self.Nlevel = [int(x) for x in self.Nlevel]
        self.active = np.ascontiguousarray(self.active, dtype=np.uint8).reshape(len(self.trans), self.Nspect)
        if self.muz.shape != self.wmu.shape:
            raise ValueError('muz and wmu must have the same shape')

    @property
    def Nspect(self): return int(self.wavelength.shape[0])
    @property
    def Nrays(self): return int(self.muz.shape[0])
    @property
    def Natoms(self): return len(self.Nlevel)
    @property
    def Ntrans(self): return len(self.trans)
    @property
    def NLtot(self): return int(sum(self.Nlevel))
    @property
    def NL2tot(self): return int(sum(n * n for n in self.Nlevel))
    @property
    def lines(self): return [t for t in self.trans if t.is_line]
    @property
    def Nlines(self): return len(self.lines)
    @property
    def SNl(self): return int(sum(t.Nlambda for t in self.lines))
    @property
    def lev_off(self): return np.concatenate([[0], np.cumsum(self.Nlevel)[:-1]]).astype(int)
    @property
    def lev2_off(self): return np.concatenate([[0], np.cumsum([n * n for n in self.Nlevel])[:-1]]).astype(int)

    def phi_shape(self):
        if self.phi_compact:
            return (self.SNl, self.Nspace)
        return (self.SNl, self.Nrays, 2, self.Nspace)

    def sca_shape(self):
        return (self.Nspect, self.Nspace) if self.sca_per_lambda else (self.Nspace,)

    def work_units_per_column(self):
        """depth-points x wavelengths x rays (both directions) per FS call."""
        return self.Nspect * self.Nrays * 2 * self.Nspace

    def to_c(self):
        """-> (LsxProblem, keepalive list)"""
        keep = []
        tarr = (_capi.LsxTransition * max(1, self.Ntrans))()
        alphas = []
        for k, t in enumerate(self.trans):
            tarr[k] = _capi.LsxTransition(t.atom, 1 if t.is_line else 0, t.i, t.j, t.Nblue, t.Nlambda,
                                          t.Aji, t.Bji, t.Bij, t.lambda0)
            if not t.is_line:
                a = f64(t.alpha, (t.Nlambda,))
                alphas.append(a)
        alpha = np.concatenate(alphas) if alphas else np.zeros(1)
        alpha = f64(alpha)
        nlevel = np.ascontiguousarray(self.Nlevel, dtype=np.int32)
        p = _capi.LsxProblem()
        p.abi_version = _capi.ABI_VERSION
        p.Nspace, p.Nrays, p.Nspect = self.Nspace, self.Nrays, self.Nspect
        p.Natoms, p.Ntrans = self.Natoms, self.Ntrans
        p.Nlevel = nlevel.ctypes.data_as(C.POINTER(C.c_int32))
        p.wavelength = _ptr(self.wavelength)
        p.muz = _ptr(self.muz)
        p.wmu = _ptr(self.wmu)
        p.trans = tarr
        p.active = self.active.ctypes.data_as(C.POINTER(C.c_uint8))
        p.alpha = _ptr(alpha)
        p.sca_per_lambda = 1 if self.sca_per_lambda else 0
        p.phi_compact = 1 if self.phi_compact else 0
        keep += [tarr, alpha, nlevel]
        return p, keep


_COLUMN_FIELDS = ('height', 'temperature', 'nStar', 'nTotal', 'n', 'C', 'bg_chi', 'bg_eta', 'bg_sca', 'phi', 'wphi')


@dataclass
class ColumnBlock:
    """Per-column inputs, leading index = column (include/lsx.h: lsx_columns)."""
    height: np.ndarray
    temperature: np.ndarray
    nStar: np.ndarray
    nTotal: np.ndarray
    n: np.ndarray
    C: np.ndarray
    bg_chi: np.ndarray
    bg_eta: np.ndarray
    bg_sca: np.ndarray
    phi: Optional[np.ndarray] = None      # None (with wphi None): Engine.set_line_profiles computes them on the device
    wphi: Optional[np.ndarray] = None

    @property
    def ncol(self):
        return int(self.height.shape[0])

    def validate(self, p: Problem):
        nc, Ns = self.ncol, p.Nspace
        shapes = dict(height=(nc, Ns), temperature=(nc, Ns), nStar=(nc, p.NLtot, Ns), nTotal=(nc, p.Natoms, Ns),
                      n=(nc, p.NLtot, Ns), C=(nc, p.NL2tot, Ns), bg_chi=(nc, p.Nspect, Ns),
                      bg_eta=(nc, p.Nspect, Ns), bg_sca=(nc,) + p.sca_shape(), phi=(nc,) + p.phi_shape(),
                      wphi=(nc, p.Nlines, Ns))
        if (self.phi is None) != (self.wphi is None):
            raise ValueError('phi and wphi must both be given or both be None')
        for k in _COLUMN_FIELDS:
            if getattr(self, k) is not None:
                setattr(self, k, f64(getattr(self, k), shapes[k]))
        return self

    def slice(self, c0, c1):
        return ColumnBlock(**{k: (None if getattr(self, k) is None else getattr(self, k)[c0:c1]) for k in _COLUMN_FIELDS})

    def to_c(self):
        s = _capi.LsxColumns()
        for k in _COLUMN_FIELDS:
            if getattr(self, k) is not None:
                setattr(s, k, _ptr(getattr(self, k)))
        return s

    @staticmethod
    def concatenate(blocks):
        return ColumnBlock(**{k: (None if getattr(blocks[0], k) is None else np.concatenate([getattr(b, k) for b in blocks]))
                              for k in _COLUMN_FIELDS})


class RadiativeRates:
    """What Engine.radiative_rates returns: .Rij, .Rji, .Rji_ref, each [ncol][Ntrans][Nspace] (Context.compute_rates: one column,
    [Ntrans][Nspace], with .transitions, the matching objects in the same order).
    Rij = sum I Vij wlamu; Rji = sum (Uji + I Vji) wlamu, the physical downward rate; Rji_ref = sum (Uji + I Vij) wlamu, the
    reference's rh_method.py:692 for one call from zero."""

    def __init__(self, Rij, Rji, Rji_ref, transitions=None, populations=None):
        self.Rij, self.Rji, self.Rji_ref = Rij, Rji, Rji_ref
        self.transitions = transitions
        self._populations = populations      # per transition (n_i, n_j), [Nspace] each

    def net(self):
        """n_j Rji - n_i Rij per transition and depth, [Ntrans][Nspace]: the net radiative bracket, from the populations the context
        held when the rates were computed"""
        if self._populations is None:
            raise ValueError('net() needs the populations: use Context.compute_rates()')
        out = np.empty_like(self.Rij)
        for kr, (ni, nj) in enumerate(self._populations):
            out[kr] = nj * self.Rji[kr] - ni * self.Rij[kr]
        return out


class RadiativeLosses:
    """What Engine.radiative_losses returns (definitions, units and signs: include/lsx_hip_losses.h); an array that was not asked
    for is None:
      .F   [ncol][Nspace]            radiative flux, W m^-2, positive towards the observer
      .Q   [ncol][Nspace]            net radiative cooling, W m^-3: positive means the gas loses energy
      .Qt  [ncol][Ntrans][Nspace]    the cooling of each transition, W m^-3, the photon energy inside the wavelength sum
      .H, .D  [ncol][Nspect][Nspace] the monochromatic Eddington flux and net emission per steradian
      .wnu [Nspect]                  the frequency weights F and Q were summed with, Hz
    Context.compute_losses drops the column axis and adds .transitions, the matching objects in the order of Qt."""
    FIELDS = ('F', 'Q', 'Qt', 'H', 'D')

    def __init__(self, wnu, F=None, Q=None, Qt=None, H=None, D=None, transitions=None):
        self.wnu = wnu
        self.F, self.Q, self.Qt, self.H, self.D = F, Q, Qt, H, D
        self.transitions = transitions

    def total(self):
        """sum over the transitions of Qt: the cooling by the active transitions alone (Q also holds the background's share and is
        summed with wnu, Qt with each transition's own weights)"""
        if self.Qt is None:
            raise ValueError("total() needs Qt: ask for it (what=('Qt', ...))")
        return self.Qt.sum(axis=-2)

    def by_transition(self, names):
        """Qt of the named transitions -> {name: [..][Nspace]}.  A name is a place in the order of Qt, one of .transitions (the
        object itself), or that object's .name where it has one"""
        if self.Qt is None:
            raise ValueError("by_transition() needs Qt: ask for it (what=('Qt', ...))")
        out = {}
        for name in ([names] if isinstance(names, (str, int, np.integer)) else list(names)):
            if isinstance(name, (int, np.integer)):
                kr = int(name)
            elif self.transitions is None:
                raise ValueError('by_transition() needs the transitions for %r: use Context.compute_losses()' % (name,))
            else:
                hits = [q for q, t in enumerate(self.transitions) if t is name or getattr(t, 'name', None) == name]
                if len(hits) != 1:
                    raise KeyError('%r names %d of the transitions' % (name, len(hits)))
                kr = hits[0]
            out[name] = self.Qt[..., kr, :]
        return out


class DepthRays:
    """What Engine.depth_rays returns: .chi, .S, .tau, .I, .contrib, each [ncol][nmu][Nspace][nla] (the wavelength runs fastest), and
    .z_tau1 [ncol][nmu][nla], for the up-going rays with direction cosines .mus and the wavelengths [.la0, .la0 + nla) of the merged
    grid; an array that was not asked for is None.  Context.compute_depth_rays drops the column axis (and the angle axis for a
    scalar mu).  Definitions: include/lsx_hip_depth.h."""
    FIELDS = ('chi', 'S', 'tau', 'I', 'contrib', 'z_tau1')

    def __init__(self, mus, la0, chi=None, S=None, tau=None, I=None, contrib=None, z_tau1=None):
        self.mus, self.la0 = mus, int(la0)
        self.chi, self.S, self.tau, self.I, self.contrib, self.z_tau1 = chi, S, tau, I, contrib, z_tau1


class StokesRays:
    """What Engine.stokes_rays returns: .I, .Q, .U, .V, each [ncol][nla][nmu], the emergent Stokes parameters of the up-going rays with
    direction cosines .mus at the wavelengths [.la0, .la0 + nla) of the merged grid.  Context.compute_stokes drops the column axis (and
    the angle axis for a scalar mu).  Definitions, the reference direction of +Q and the sign of V: include/lsx_hip_stokes.h."""
    FIELDS = ('I', 'Q', 'U', 'V')

    def __init__(self, mus, la0, I, Q, U, V):
        self.mus, self.la0 = mus, int(la0)
        self.I, self.Q, self.U, self.V = I, Q, U, V


class StokesResponse:
    """What Engine.stokes_response returns: .rf, a dict from the names of the requested parameters ('B', 'gammaB', 'chiB') to
    [ncol][4][nla][nk][nmu] arrays (the responses of I, Q, U, V to that parameter at the depths .ks, per tesla resp. per radian),
    .stokes, the StokesRays of the call's own field, and .ks, .mus, .la0, .amplitudes (a dict like .rf).
    Context.compute_stokes_response drops the column axis (and the angle axis for a scalar mu).
    Definitions: include/lsx_hip_stokes_response.h."""
    PARAMETERS = ('B', 'gammaB', 'chiB')
    DEFAULT_AMPLITUDES = {'B': 1e-3, 'gammaB': 1e-3, 'chiB': 1e-3}          # T, rad, rad
    # with the velocity of the call (include/lsx_hip_stokes_velocity.h): 'vlos' is the fourth parameter, per m/s
    VELOCITY_PARAMETERS = PARAMETERS + ('vlos',)
    VELOCITY_DEFAULT_AMPLITUDES = dict(DEFAULT_AMPLITUDES, vlos=100.0)       # ..., m/s

    def __init__(self, rf, stokes, ks, mus, la0, amplitudes):
        self.rf, self.stokes, self.ks, self.mus, self.la0, self.amplitudes = rf, stokes, ks, mus, int(la0), amplitudes


class NgOptions:
    """Ng acceleration of the MALI loop (include/lsx_hip_ng.h): order 1 or 2 (0: off), delay >= 0 statistical equilibria that pass
    before the first population vector is stored.  What Context(ng=...) and run_response_function(ng=...) take."""
    __slots__ = ('order', 'delay')

    def __init__(self, order=2, delay=0):
        order, delay = int(order), int(delay)
        if order not in (0, 1, 2):
            raise ValueError('NgOptions: order %d; 1 and 2 are offered, 0 switches it off' % order)
        if delay < 0:
            raise ValueError('NgOptions: delay %d is negative' % delay)
        self.order, self.delay = order, delay

    def __eq__(self, other):
        return isinstance(other, NgOptions) and (self.order, self.delay) == (other.order, other.delay)

    def __hash__(self):
        return hash((self.order, self.delay))

    def __repr__(self):
        return 'NgOptions(order=%d, delay=%d)' % (self.order, self.delay)


class NgState:
    """What Engine.ng_state returns: .stored, .applied, .rejected, int32 [ncol]; .coef [ncol][Natoms][2], the coefficients of each
    column's last step taken (include/lsx_hip_ng.h)"""

    def __init__(self, stored, applied, rejected, coef):
        self.stored, self.applied, self.rejected, self.coef = stored, applied, rejected, coef


class Engine:
    """One lsx_ctx.  `lib=None` binds the HIP backend (and raises if it is not built)."""
    _serials = itertools.count(1)

    def __init__(self, problem: Problem, ncol: int, device: int = 0, stream: Optional[int] = None, lib=None,
                 policy_columns: Optional[int] = None, sweep_policy: str = 'auto', options=None):
        """policy_columns: the column count of the WHOLE problem this engine holds a shard of (None: its own `ncol`).  The HIP
        library picks its sweep kernel by a column count; a driver that splits N columns over several engines passes N to all
        of them, so that every column gets the bits it gets when all N sit in one engine (include/lsx.h, lsx_set_sweep_policy).
        options: explicit plan / runtime switches, "key=value,..." or a dict (include/lsx.h, lsx_create_with_options); what the
        engine ended up with: effective_options() / options_signature()."""
        self.lib = lib if lib is not None else _capi.load_hip_library()
        self.serial = next(Engine._serials)      # this process's n-th engine: what per-engine bookkeeping keys on (never re-used, unlike id())
        self.problem = problem
        self.ncol = int(ncol)
        self._have_atomic_data = False
        self._h = C.c_void_p()
        cprob, self._keep = problem.to_c()
        if isinstance(options, dict):
            options = ','.join('%s=%s' % (k, int(v) if isinstance(v, bool) else v) for k, v in options.items())
        if getattr(self.lib, 'old_abi', False) and not options:
            self.lib.check(self.lib.dll.lsx_create(C.byref(cprob), self.ncol, int(device), C.c_void_p(stream) if stream else None, C.byref(self._h)))
        else:
            self.lib.check(self.lib.dll.lsx_create_with_options(C.byref(cprob), self.ncol, int(device), C.c_void_p(stream) if stream else None,
                                                                options.encode() if options else None, C.byref(self._h)))
        if policy_columns is not None or sweep_policy != 'auto':
            self.set_sweep_policy(sweep_policy, policy_columns)

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self.lib.dll.lsx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- data in --------------------------------------------------------------
    def set_columns(self, col0: int, block: ColumnBlock):
        block.validate(self.problem)
        cs = block.to_c()
        self.lib.check(self.lib.dll.lsx_set_columns(self._h, int(col0), block.ncol, C.byref(cs)))

    def set_line_profiles(self, col0, aDamp, vBroad, vlos=None):
        """ComputationalTransition.compute_phi (rh_method.py:198-243) on the device, for columns
        [col0, col0 + ncol): aDamp [ncol][Nlines][Nspace], vBroad [ncol][Natoms][Nspace], vlos [ncol][Nspace]."""
        p = self.problem
        aDamp = f64(aDamp)
        ncol = aDamp.shape[0]
        aDamp = f64(aDamp, (ncol, p.Nlines, p.Nspace))
        vBroad = f64(vBroad, (ncol, p.Natoms, p.Nspace))
        vl = None if vlos is None else f64(vlos, (ncol, p.Nspace))
        self.lib.check(self.lib.dll.lsx_set_line_profiles(self._h, int(col0), ncol, _ptr(aDamp), _ptr(vBroad),
                                                          _ptr(vl) if vl is not None else None))

    def set_atomic_data(self, data):
        """atomdata.AtomicData -> lsx_set_atomic_data (once per engine, before set_atmosphere)"""
        cd, keep = data.to_c()
        self.lib.check(self.lib.dll.lsx_set_atomic_data(self._h, C.byref(cd)))
        del keep
        self._have_atomic_data = True

    def setup_columns(self, col0, model, setup, start_n=None):
        """Columns [col0, col0 + model.ncol) from their atmosphere to a ready context, entirely through device entries
        (native.setup_columns): placeholder set_columns, convert_scales(install), background(install), eq_pops for hydrogen and the
        active atoms, set_atmosphere(lte_pops=True), and set(LSX_N, start_n) for a warm start.  model: native.ColumnModel; setup:
        native.NativeSetup.  set_atomic_data is done on first use."""
        from .native import setup_columns
        return setup_columns(self, col0, model, setup, start_n=start_n)

    def set_atmosphere(self, col0, temperature, ne, vturb, nHGround, nTotal, vlos=None, lte_pops=False):
        """lsx_set_atmosphere for columns [col0, col0 + ncol): the library derives vBroad, aDamp, the line profiles, the
        collisional rates and (lte_pops) the LTE populations from the atmosphere (rh_method.py:198-243, 474-487;
        atomic_model.py:66-69, 491-502; atomic_set.py:105-145).  Arrays [ncol][Nspace]; nTotal [ncol][Natoms][Nspace]."""
        p = self.problem
        T = f64(temperature)
        ncol = T.shape[0]
        T = f64(T, (ncol, p.Nspace))
        arrs = dict(temperature=T, ne=f64(ne, (ncol, p.Nspace)), vturb=f64(vturb, (ncol, p.Nspace)),
                    nHGround=f64(nHGround, (ncol, p.Nspace)), nTotal=f64(nTotal, (ncol, p.Natoms, p.Nspace)))
        if vlos is not None:
            arrs['vlos'] = f64(vlos, (ncol, p.Nspace))
        a = _capi.LsxAtmosphere()
        for k, v in arrs.items():
            setattr(a, k, _ptr(v))
        a.lte_pops = 1 if lte_pops else 0
        self.lib.check(self.lib.dll.lsx_set_atmosphere(self._h, int(col0), ncol, C.byref(a)))

    def set(self, what, arr, col0=0):
        arr = f64(arr)
        ncol = arr.shape[0]
        self.lib.check(self.lib.dll.lsx_set(self._h, what, int(col0), ncol, _ptr(arr), arr.nbytes))

    def set_formal_solver(self, solver):
        """'linear' (the reference's piecewise_linear_1d, default) or 'parabolic' (monotonic piecewise parabolic, include/lsx.h N4)"""
        kind = {'linear': _capi.LSX_SOLVER_LINEAR, 'parabolic': _capi.LSX_SOLVER_PARABOLIC}[solver]
        self.lib.check(self.lib.dll.lsx_set_formal_solver(self._h, kind))

    def set_sweep_policy(self, policy='auto', decide_for_columns=None):
        """'auto' (by column count: `decide_for_columns`, default this engine's own), 'ray-per-lane' or 'ray-serial'"""
        kind = {'auto': _capi.LSX_SWEEP_AUTO, 'ray-per-lane': _capi.LSX_SWEEP_RAY_PER_LANE,
                'ray-serial': _capi.LSX_SWEEP_RAY_SERIAL}[policy]
        self.lib.check(self.lib.dll.lsx_set_sweep_policy(self._h, kind, int(decide_for_columns or 0)))

    def effective_options(self) -> str:
        """everything that decides how this engine associates its sums and launches its kernels: the options it was created with
        (environment defaults + explicit list), the rule, the sweep mapping the policy selects, the plan's class list"""
        for size in (4096, 1 << 16, 1 << 20):        # (the class list grows with the plan: include/lsx.h)
            buf = C.create_string_buffer(size)
            if self.lib.dll.lsx_effective_options(self._h, buf, size) == 0:
                return buf.value.decode()
        self.lib.check(self.lib.dll.lsx_effective_options(self._h, buf, size))
        return buf.value.decode()

    def options_signature(self) -> int:
        """64-bit hash of effective_options(): engines with equal signatures on equal problems give every column the same bits"""
        return int(self.lib.dll.lsx_options_signature(self._h))

    def sweep_policy(self) -> str:
        """the mapping the next formal solution runs -- under the parabolic rule: for the classes that have a ray-serial instance of it
        ('oracle' for the CPU restatement, which has one code path)"""
        return {0: 'oracle', 1: 'ray-per-lane', 2: 'ray-serial'}[int(self.lib.dll.lsx_sweep_policy(self._h))]

    def set_active_columns(self, mask=None):
        """freeze columns whose mask entry is False (None: all active)"""
        if mask is None:
            self.lib.check(self.lib.dll.lsx_set_active_columns(self._h, None))
            return
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if m.shape != (self.ncol,):
            raise ValueError('mask must have one entry per column')
        self.lib.check(self.lib.dll.lsx_set_active_columns(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8))))

    # -- hot path -------------------------------------------------------------
    def formal_sol_gamma(self) -> float:
        v = C.c_double()
        self.lib.check(self.lib.dll.lsx_formal_sol_gamma(self._h, C.byref(v)))
        return v.value

    def stat_equil(self) -> float:
        v = C.c_double()
        self.lib.check(self.lib.dll.lsx_stat_equil(self._h, C.byref(v)))
        return v.value

    def formal_sol_gamma_async(self):
        self.lib.check(self.lib.dll.lsx_formal_sol_gamma_async(self._h))

    def stat_equil_async(self):
        self.lib.check(self.lib.dll.lsx_stat_equil_async(self._h))

    def sync(self):
        a, b = C.c_double(), C.c_double()
        self.lib.check(self.lib.dll.lsx_sync(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- the loop without a host round trip per iteration (include/lsx.h; drivers.iterate_mali_engine) ----
    def sync_begin(self, populations=False):
        """enqueue the read-back of the monitors of the calls enqueued so far (populations: and of n, for fetch_populations)"""
        if populations:
            self.lib.check(self.lib.dll.lsx_sync_begin_populations(self._h))
        else:
            self.lib.check(self.lib.dll.lsx_sync_begin(self._h))

    def fetch_populations(self):
        """the populations [ncol][NLtot][Nspace] as the last collected sync_begin(populations=True) read them back -- host to host:
        it does not wait for what has been enqueued behind that read-back"""
        out = np.empty((self.ncol,) + self._shape(_capi.LSX_N), dtype=np.float64)
        self.lib.check(self.lib.dll.lsx_fetch_populations(self._h, _ptr(out), out.nbytes))
        return out

    def sync_end(self):
        """-> (dJ, dPops) of that read-back; what was enqueued behind it keeps running"""
        a, b = C.c_double(), C.c_double()
        self.lib.check(self.lib.dll.lsx_sync_end(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def formal_sol_gamma_speculative(self):
        """the next iteration's formal solution, enqueued before the monitors of this one are known"""
        self.lib.check(self.lib.dll.lsx_formal_sol_gamma_speculative(self._h))

    def prefers_lookahead(self) -> bool:
        """whether enqueueing ahead pays for this context (include/lsx.h, lsx_prefers_lookahead)"""
        return bool(self.lib.dll.lsx_prefers_lookahead(self._h))

    def discard_formal_sol(self):
        """take the speculative formal solution back: I, J, Gamma and the monitors are the previous call's again"""
        self.lib.check(self.lib.dll.lsx_discard_formal_sol(self._h))

    def monitors_to(self, ptr):
        """lsx_monitors: (max dJ, max dPops, NaN flag, singular flag) of the enqueued calls -> 4 doubles at `ptr`
        (an int address: device memory for the HIP library -- e.g. tensor.data_ptr() -- host memory for the oracle)"""
        self.lib.check(self.lib.dll.lsx_monitors(self._h, C.c_void_p(int(ptr))))

    def time_formal_sol(self, warmup, reps):
        a, b = C.c_double(), C.c_double()
        self.lib.check(self.lib.dll.lsx_time_formal_sol(self._h, int(warmup), int(reps), C.byref(a), C.byref(b)))
        return a.value, b.value

    def algorithmic_bytes_per_column(self) -> float:
        return float(self.lib.dll.lsx_algorithmic_bytes_per_column(self._h))

    # -- data out -------------------------------------------------------------
    def _shape(self, what):
        p = self.problem
        return {_capi.LSX_I: (p.Nspect, p.Nrays), _capi.LSX_J: (p.Nspect, p.Nspace),
                _capi.LSX_N: (p.NLtot, p.Nspace), _capi.LSX_GAMMA: (p.NL2tot, p.Nspace),
                _capi.LSX_DJ_COL: (), _capi.LSX_DPOPS_COL: (), _capi.LSX_NSTAR: (p.NLtot, p.Nspace),
                _capi.LSX_C: (p.NL2tot, p.Nspace), _capi.LSX_PHI: p.phi_shape(),
                _capi.LSX_WPHI: (p.Nlines, p.Nspace), _capi.LSX_VBROAD: (p.Natoms, p.Nspace),
                _capi.LSX_ADAMP: (max(1, p.Nlines), p.Nspace)}[what]

    def get(self, what, col0=0, ncol=None):
        ncol = self.ncol - col0 if ncol is None else ncol
        out = np.empty((ncol,) + self._shape(what), dtype=np.float64)
        self.lib.check(self.lib.dll.lsx_get(self._h, what, int(col0), int(ncol), _ptr(out), out.nbytes))
        return out

    # -- the entries of the HIP library alone (include/lsx_hip*.h; _capi.HIP_FEATURES): what their wrappers below share --
    def _need(self, feature, entry):
        """NotImplementedError naming `entry` where the library (or what stands in for one) lacks the feature"""
        if not getattr(self.lib, 'has_' + feature, False):
            _capi.LsxLibrary.missing(self.lib, feature, entry)

    def _work_cap(self, entry, nbytes):
        if nbytes is not None:
            self.lib.check(getattr(self.lib.dll, entry)(self._h, int(nbytes)))

    def _columns(self, col0, ncol):
        return self.ncol - int(col0) if ncol is None else int(ncol)

    def _window(self, la0, nla):
        return self.problem.Nspect - int(la0) if nla is None else int(nla)

    def _per_depth(self, a, nc):
        """a scalar, [Nspace] or [nc][Nspace] -> [nc][Nspace]"""
        return f64(np.broadcast_to(np.asarray(a, dtype=np.float64), (nc, self.problem.Nspace)))

    @staticmethod
    def _amplitudes(nq, amplitudes):
        """-> (the amplitude of every parameter by name, those of the first nq of B, gammaB, chiB, vlos as the array the entries take)"""
        amps = dict(StokesResponse.VELOCITY_DEFAULT_AMPLITUDES if nq == 4 else StokesResponse.DEFAULT_AMPLITUDES)
        amps.update(amplitudes or {})
        return amps, f64(np.array([amps[w] for w in StokesResponse.VELOCITY_PARAMETERS[:nq]], dtype=np.float64))

    def epilogue_info(self):
        """Launch counters of the kernels behind the sweep since the engine was made (include/lsx_hip_epilogue.h; HIP library only):
        -> dict(rows={(lanes per depth row, threads, segmented): launches of the row-mapped fast-continuum epilogue, launched ones only},
        cols=[launches per column-mapped tile list], prepass=(whole column, segmented), finish=dict(small=, levels=, lds=), finish_nt=)."""
        self._need('epilogue_info', 'lsx_hip_epilogue_info')
        out = (C.c_int64 * 64)()
        n = self.lib.dll.lsx_hip_epilogue_info(self._h, out)
        assert n == 49, n
        v = [int(x) for x in out[:n]]
        rows = {(v[i] >> 10, (v[i] & 1023) >> 1, bool(v[i] & 1)): v[i + 1] for i in range(0, 36, 2) if v[i + 1]}
        return dict(rows=rows, cols=v[36:43], prepass=(v[43], v[44]), finish=dict(small=v[45], levels=v[46], lds=v[47]), finish_nt=v[48])

    def emergent_rays(self, mus, col0=0, ncol=None):
        """Emergent intensity at arbitrary viewing angles from what the engine holds (include/lsx_hip.h, lsx_hip_emergent_rays):
        one final-pass formal solution of the up-going rays with direction cosines `mus` (each in (0, 1], any number of them)
        for columns [col0, col0 + ncol), from the current populations and J.  Read-only.  -> [ncol][Nspect][nmu].
        Only the HIP library computes it; there is no host version."""
        self._need('emergent_rays', 'lsx_hip_emergent_rays')
        mu, ncol = _vector(mus), self._columns(col0, ncol)
        out = np.empty((max(ncol, 0), self.problem.Nspect, mu.shape[0]), dtype=np.float64)
        self.lib.check(self.lib.dll.lsx_hip_emergent_rays(self._h, mu.shape[0], _ptr(mu), int(col0), ncol, _ptr(out), out.nbytes))
        return out

    def emergent_spectrum(self, mus, wavelength, alpha=None, bg_chi=None, bg_eta=None, bg_sca=None, col0=0, ncol=None,
                          work_cap_bytes=None):
        """Emergent intensity at arbitrary WAVELENGTHS (nm, strictly ascending; they need not be points of the problem's grid) and
        viewing angles from what the engine holds (include/lsx_hip_spectrum.h, lsx_hip_spectrum), for columns [col0, col0 + ncol),
        from the current populations and J.  alpha: [Ncont][nla], every continuum's cross-section at `wavelength` (continua in
        table order; None only without continua).  bg_chi, bg_eta (and bg_sca in a sca_per_lambda problem): [ncol][nla][Nspace],
        the background at `wavelength`; all None: the engine's own background is interpolated between its grid points (an
        approximation between them).  J is interpolated likewise, always.
        work_cap_bytes: the cap of the pass's device memory from this call on (None: unchanged; 0: the default).
        Read-only.  -> [ncol][nla][nmu].  Only the HIP library computes it; there is no host version."""
        self._need('spectrum', 'lsx_hip_spectrum')
        self._work_cap('lsx_hip_spectrum_work_cap', work_cap_bytes)
        mu, w, ncol = _vector(mus), _vector(wavelength), self._columns(col0, ncol)
        nla = w.shape[0]
        Ncont = self.problem.Ntrans - self.problem.Nlines
        al = None if alpha is None else f64(alpha, (Ncont, nla))
        bg = [None if a is None else f64(a, (max(ncol, 0), nla, self.problem.Nspace)) for a in (bg_chi, bg_eta, bg_sca)]
        out = np.empty((max(ncol, 0), nla, mu.shape[0]), dtype=np.float64)
        self.lib.check(self.lib.dll.lsx_hip_spectrum(self._h, nla, _ptr(w), _opt(al), _opt(bg[0]), _opt(bg[1]), _opt(bg[2]), mu.shape[0],
                                                     _ptr(mu), int(col0), ncol, _ptr(out), out.nbytes))
        return out

    def radiative_rates(self, col0=0, ncol=None, work_cap_bytes=None):
        """Radiative rates of every transition from what the engine holds (include/lsx_hip_rates.h, lsx_hip_radiative_rates): one
        formal solution over the engine's own rays from the current populations and J, for columns [col0, col0 + ncol).
        Read-only; nothing is accumulated over calls.  -> RadiativeRates with .Rij, .Rji (physical: Vji in the stimulated term) and
        .Rji_ref (the reference's rh_method.py:692 for one call), each [ncol][Ntrans][Nspace], transitions in table order.
        work_cap_bytes: the cap of the pass's device work memory from this call on (None: unchanged; 0: the default).
        Only the HIP library computes it; there is no host version."""
        self._need('radiative_rates', 'lsx_hip_radiative_rates')
        self._work_cap('lsx_hip_radiative_rates_work_cap', work_cap_bytes)
        ncol = self._columns(col0, ncol)
        shape = (max(ncol, 0), self.problem.Ntrans, self.problem.Nspace)
        Rij, Rji, Rji_ref = (np.empty(shape, dtype=np.float64) for _ in range(3))
        self.lib.check(self.lib.dll.lsx_hip_radiative_rates(self._h, int(col0), ncol, _ptr(Rij), _ptr(Rji), _ptr(Rji_ref), Rij.nbytes))
        return RadiativeRates(Rij, Rji, Rji_ref)

    def frequency_weights(self):
        """the weights radiative_losses uses by default: the trapezoid rule in frequency over the merged grid, [Nspect] in Hz
        (lsx_hip_frequency_weights, formed in the library's grid code)"""
        self._need('radiative_losses', 'lsx_hip_frequency_weights')
        lam = f64(self.problem.wavelength)
        w = np.empty_like(lam)
        self.lib.check(self.lib.dll.lsx_hip_frequency_weights(lam.shape[0], _ptr(lam), _ptr(w)))
        return w

    def radiative_losses(self, col0=0, ncol=None, wnu=None, what=('F', 'Q', 'Qt'), work_cap_bytes=None):
        """What the radiation does to the gas, from what the engine holds (include/lsx_hip_losses.h, lsx_hip_radiative_losses): one
        formal solution over the engine's own rays from the current populations and J, for columns [col0, col0 + ncol).
        -> RadiativeLosses with the arrays named in `what`, of 'F' (flux, W m^-2, positive outwards), 'Q' (net cooling, W m^-3,
        positive: the gas loses energy), 'Qt' (per transition), 'H', 'D' (monochromatic), and .wnu, the weights used.
        wnu: [Nspect] frequency weights in Hz for F and Q (None: the trapezoid rule over the merged grid); zeros outside a band give
        the band's share.  work_cap_bytes: the cap of the pass's device work memory from this call on (None: unchanged; 0: the
        default).  Read-only.  Only the HIP library computes it; there is no host version."""
        self._need('radiative_losses', 'lsx_hip_radiative_losses')
        what = (what,) if isinstance(what, str) else tuple(what)
        unknown = [w for w in what if w not in RadiativeLosses.FIELDS]
        if unknown:
            raise ValueError('radiative_losses: unknown array(s) %s; there are %s' % (unknown, ', '.join(RadiativeLosses.FIELDS)))
        self._work_cap('lsx_hip_radiative_losses_work_cap', work_cap_bytes)
        p, ncol = self.problem, self._columns(col0, ncol)
        nc = max(ncol, 0)
        shapes = {'F': (nc, p.Nspace), 'Q': (nc, p.Nspace), 'Qt': (nc, p.Ntrans, p.Nspace), 'H': (nc, p.Nspect, p.Nspace),
                  'D': (nc, p.Nspect, p.Nspace)}
        out = {w: np.empty(shapes[w], dtype=np.float64) for w in what}
        weights = self.frequency_weights() if wnu is None else f64(wnu, (p.Nspect,))
        ptr = [_ptr(out[w]) if w in out else None for w in RadiativeLosses.FIELDS]
        nbytes = [int(np.prod(shapes[w])) * 8 for w in ('F', 'Qt', 'H')]
        self.lib.check(self.lib.dll.lsx_hip_radiative_losses(self._h, int(col0), ncol, None if wnu is None else _ptr(weights), *ptr,
                                                             *nbytes))
        return RadiativeLosses(weights, **out)

    def depth_rays(self, mus, la0=0, nla=None, col0=0, ncol=None, what=DepthRays.FIELDS, work_cap_bytes=None):
        """Opacity, source function, optical depth, intensity and contribution function at every depth along the up-going rays with
        direction cosines `mus`, and the height of tau = 1 (include/lsx_hip_depth.h, lsx_hip_depth_rays), for columns
        [col0, col0 + ncol) and the wavelengths [la0, la0 + nla) of the merged grid (nla None: to the end of the grid), from the
        current populations and J.  Read-only.  what: the arrays wanted, of 'chi', 'S', 'tau', 'I', 'contrib', 'z_tau1'.
        work_cap_bytes: the cap of the pass's device memory from this call on (None: unchanged; 0: the default).
        -> DepthRays.  Only the HIP library computes it; there is no host version."""
        self._need('depth_rays', 'lsx_hip_depth_rays')
        what = (what,) if isinstance(what, str) else tuple(what)
        unknown = [w for w in what if w not in DepthRays.FIELDS]
        if unknown:
            raise ValueError('depth_rays: unknown array(s) %s; there are %s' % (unknown, ', '.join(DepthRays.FIELDS)))
        self._work_cap('lsx_hip_depth_rays_work_cap', work_cap_bytes)
        mu, ncol, nla = _vector(mus), self._columns(col0, ncol), self._window(la0, nla)
        shape = (max(ncol, 0), mu.shape[0], self.problem.Nspace, max(nla, 0))
        out = {w: np.empty(shape[:2] + shape[3:] if w == 'z_tau1' else shape, dtype=np.float64) for w in what}
        ptr = [_ptr(out[w]) if w in out else None for w in DepthRays.FIELDS]
        self.lib.check(self.lib.dll.lsx_hip_depth_rays(self._h, mu.shape[0], _ptr(mu), int(col0), ncol, int(la0), nla, *ptr,
                                                       int(np.prod(shape)) * 8, int(np.prod(shape[:2] + shape[3:])) * 8))
        return DepthRays(mu, la0, **out)

    def _stokes_prefix(self, mus, B, gammaB, chiB, patterns, la0, nla, col0, ncol):
        """what the entries of stokes_rays and stokes_response begin with: handle, angles, columns, window, the three fields, the four
        pattern arrays -> (those 14 arguments, what must outlive the call, mu, the columns and the wavelengths of the outputs)"""
        from . import zeeman
        mu, ncol, nla = _vector(mus), self._columns(col0, ncol), self._window(la0, nla)
        nc = max(ncol, 0)
        fld = [self._per_depth(a, nc) for a in (B, gammaB, chiB)]
        ncomp, alpha, strength, shift = zeeman.pack(patterns, self.problem.Nlines)
        args = (self._h, mu.shape[0], _ptr(mu), int(col0), ncol, int(la0), nla, _ptr(fld[0]), _ptr(fld[1]), _ptr(fld[2]), _iptr(ncomp),
                _iptr(alpha), _ptr(strength), _ptr(shift))
        return args, (mu, fld, ncomp, alpha, strength, shift), mu, nc, max(nla, 0)

    def stokes_rays(self, mus, B, gammaB, chiB, patterns=None, la0=0, nla=None, col0=0, ncol=None, work_cap_bytes=None, vlos=None):
        """Emergent Stokes spectra in a magnetic field (Zeeman effect, field-free method: include/lsx_hip_stokes.h,
        lsx_hip_stokes_rays) of the up-going rays with direction cosines `mus`, for columns [col0, col0 + ncol) and the wavelengths
        [la0, la0 + nla) of the merged grid (nla None: to the end), from the current populations and J.  B [T], gammaB, chiB [rad]:
        [ncol][Nspace] (a single column may be 1-D, a scalar holds everywhere): strength, inclination against the vertical, azimuth.
        patterns: one entry per LINE of the problem in table order -- None (unpolarised), a zeeman.ZeemanComponents or an
        (alpha, strength, shift) triple; None: no line is polarised.  work_cap_bytes: the cap of the pass's device memory from this
        call on (None: unchanged; 0: the default).  vlos [m/s], shaped like B: the line-of-sight velocity of this call in the place of
        the context's (include/lsx_hip_stokes_velocity.h, lsx_hip_velocity_stokes_rays; populations and J do not follow it); None: the
        context's own.  Read-only.  -> StokesRays.  Only the HIP library computes it."""
        self._need('stokes', 'lsx_hip_stokes_rays')
        self._work_cap('lsx_hip_stokes_rays_work_cap', work_cap_bytes)
        args, _keep, mu, nc, nla = self._stokes_prefix(mus, B, gammaB, chiB, patterns, la0, nla, col0, ncol)
        out = np.empty((nc, 4, nla, mu.shape[0]), dtype=np.float64)
        args += (_ptr(out), out.nbytes)
        if vlos is None:
            self.lib.check(self.lib.dll.lsx_hip_stokes_rays(*args))
        else:
            self._need('stokes_velocity', 'lsx_hip_velocity_stokes_rays')
            vl = self._per_depth(vlos, nc)
            self.lib.check(self.lib.dll.lsx_hip_velocity_stokes_rays(*args, _ptr(vl)))
        return StokesRays(mu, la0, out[:, 0], out[:, 1], out[:, 2], out[:, 3])

    def stokes_response(self, mus, B, gammaB, chiB, patterns=None, la0=0, nla=None, col0=0, ncol=None,
                        parameters=StokesResponse.PARAMETERS, amplitudes=None, ks=None, work_cap_bytes=None, vlos=None):
        """Response functions of the emergent Stokes vector to the field strength, inclination and azimuth at every depth
        (include/lsx_hip_stokes_response.h, lsx_hip_response_stokes): RF_p[k] = (S(p_k + a_p / 2) - S(p_k - a_p / 2)) / a_p, S what
        stokes_rays returns for the field changed at depth k of that column alone.  Arguments as stokes_rays, then
        parameters: some of 'B', 'gammaB', 'chiB'; amplitudes: a dict from those names to a_p (None, or a name left out: 1e-3 T,
        1e-3 rad); ks: the depths, strictly increasing (None: all).  B must be at least a_B / 2 at every requested depth where 'B'
        is requested.  vlos [m/s], shaped like B: the velocity of this call as in stokes_rays; with it, or alone, 'vlos' may be among
        the parameters (include/lsx_hip_stokes_velocity.h, lsx_hip_velocity_response_stokes; amplitude 100 m/s unless given) -- where
        'vlos' is requested and no velocity is given, the velocity is zero.  Read-only.  -> StokesResponse.  Only the HIP library
        computes it."""
        self._need('stokes_response', 'lsx_hip_response_stokes')
        self._work_cap('lsx_hip_response_stokes_work_cap', work_cap_bytes)
        names = [parameters] if isinstance(parameters, str) else list(parameters)
        vel = vlos is not None or 'vlos' in names
        known = StokesResponse.VELOCITY_PARAMETERS if vel else StokesResponse.PARAMETERS
        for w in names:
            if w not in StokesResponse.VELOCITY_PARAMETERS:
                raise ValueError("stokes_response: parameter %r is not one of 'B', 'gammaB', 'chiB', 'vlos'" % (w,))
        names = [w for w in known if w in names]
        amps, amp = self._amplitudes(len(known), amplitudes)
        bits = sum(1 << known.index(w) for w in names)
        args, _keep, mu, nc, nla = self._stokes_prefix(mus, B, gammaB, chiB, patterns, la0, nla, col0, ncol)
        Ns = self.problem.Nspace
        kk = None if ks is None else np.ascontiguousarray(np.asarray(ks).reshape(-1), dtype=np.int32)
        nk = Ns if kk is None else kk.shape[0]
        rf = np.empty((nc, len(names), 4, nla, nk, mu.shape[0]), dtype=np.float64)
        out = np.empty((nc, 4, nla, mu.shape[0]), dtype=np.float64)
        args += (bits, _ptr(amp), nk, None if kk is None else _iptr(kk), _ptr(rf), rf.nbytes, _ptr(out), out.nbytes)
        if not vel:
            self.lib.check(self.lib.dll.lsx_hip_response_stokes(*args))
        else:
            self._need('stokes_velocity', 'lsx_hip_velocity_response_stokes')
            vl = self._per_depth(0.0 if vlos is None else vlos, nc)
            self.lib.check(self.lib.dll.lsx_hip_velocity_response_stokes(*args, _ptr(vl)))
        return StokesResponse({w: rf[:, i] for i, w in enumerate(names)}, StokesRays(mu, la0, out[:, 0], out[:, 1], out[:, 2], out[:, 3]),
                              np.arange(Ns, dtype=np.int32) if kk is None else kk, mu, la0, {w: float(amps[w]) for w in names})

    def _instrument(self, who, instrument, nla):
        """-> (the C struct of a fit.Instrument, what must outlive the call)"""
        self._need('fit_instrument', 'lsx_hip_instrument_fit_normal')
        if instrument.nla != nla:
            raise ValueError('%s: the instrument is made for %d wavelengths, the window has %d' % (who, instrument.nla, nla))
        first, weight = instrument.first, instrument.weight
        return _capi.LsxFitInstrument(instrument.nobs, instrument.width, _iptr(first), _ptr(weight)), (first, weight)

    def apply_instrument(self, x, instrument):
        """The instrument applied on the device, by the kernel the fit runs (include/lsx_hip_fit_instrument.h,
        lsx_hip_instrument_apply): x [...][nla][nmu] -> [...][nobs][nmu], e.g. the [ncol][4][nla][nmu] of stokes_rays stacked.  What
        the fit forms inside for the same numbers, bit for bit.  Does not touch the engine's state."""
        a = f64(np.asarray(x, dtype=np.float64))
        if a.ndim < 2:
            raise ValueError('apply_instrument: x must be [...][nla][nmu]')
        nla, nmu = a.shape[-2:]
        st, keep = self._instrument('apply_instrument', instrument, nla)
        nrow = int(np.prod(a.shape[:-2]))
        out = np.empty(a.shape[:-2] + (instrument.nobs, nmu), dtype=np.float64)
        self.lib.check(self.lib.dll.lsx_hip_instrument_apply(self._h, C.byref(st), nla, nmu, nrow, _ptr(a), _ptr(out)))
        del keep
        return out

    def _fit_args(self, kind, mus, basis, nnode, nodes, obs, weight, base, patterns, la0, nla, col0, ncol, work_cap_bytes, instrument=None):
        """what fit_field_normal and fit_field_chi2 (kind 'normal' / 'chi2') share: the checks and the 15 arguments their entries begin with"""
        from . import zeeman
        who = 'fit_field_' + kind
        self._need('fit_field', 'lsx_hip_fit_field_' + kind)
        self._work_cap('lsx_hip_fit_field_work_cap', work_cap_bytes)
        mu, ncol, nla = _vector(mus), self._columns(col0, ncol), self._window(la0, nla)
        nc, Ns = max(ncol, 0), self.problem.Nspace
        nn = np.ascontiguousarray(np.asarray(nnode).reshape(-1), dtype=np.int32)
        if nn.shape[0] not in (3, 4):
            raise ValueError('%s: nnode must hold three counts (B, gammaB, chiB) or four (then vlos)' % who)
        nq = nn.shape[0]
        if nq == 4:
            self._need('stokes_velocity', 'lsx_hip_velocity_fit_' + kind)
        P = max(int(nn.clip(min=0).sum()), 1)
        bas = f64(np.asarray(basis, dtype=np.float64).reshape(-1, Ns))
        if bas.shape[0] != int(nn.sum()):
            raise ValueError('%s: basis has %d rows, nnode sums to %d' % (who, bas.shape[0], int(nn.sum())))
        x = f64(np.broadcast_to(np.asarray(nodes, dtype=np.float64), (nc, P)))
        shape = (nc, 4, max(nla, 0) if instrument is None else instrument.nobs, mu.shape[0])
        ob = f64(np.asarray(obs, dtype=np.float64).reshape(shape))
        wt = None if weight is None else f64(np.broadcast_to(np.asarray(weight, dtype=np.float64), shape))
        bs = None if base is None else f64(np.broadcast_to(np.asarray(base, dtype=np.float64), (nc, nq, Ns)))
        ncomp, alpha, strength, shift = zeeman.pack(patterns, self.problem.Nlines)
        keep = (mu, nn, bas, x, ob, wt, bs, ncomp, alpha, strength, shift)
        head = [self._h, mu.shape[0], _ptr(mu), int(col0), ncol, int(la0), nla, _iptr(ncomp), _iptr(alpha), _ptr(strength), _ptr(shift),
                _iptr(nn), _ptr(bas), _opt(bs), _ptr(x)]
        return head, keep, _ptr(ob), _opt(wt), nc, P, Ns, nq

    def _fit_call(self, kind, head, tail, nq, instrument):
        """the one place that picks the entry of a fit: lsx_hip_fit_field_<kind> for three quantities and no instrument,
        lsx_hip_instrument_fit_<kind> with one, lsx_hip_velocity_fit_<kind> for four quantities, its last argument the instrument or NULL"""
        if nq == 3 and instrument is None:
            self.lib.check(getattr(self.lib.dll, 'lsx_hip_fit_field_' + kind)(*head, *tail))
            return
        st, keep = (None, None) if instrument is None else self._instrument('fit_field_' + kind, instrument, head[6])
        entry = getattr(self.lib.dll, ('lsx_hip_velocity_fit_' if nq == 4 else 'lsx_hip_instrument_fit_') + kind)
        self.lib.check(entry(*head, *tail, None if st is None else C.byref(st)))
        del keep

    def fit_field_normal(self, mus, basis, nnode, nodes, obs, weight=None, base=None, patterns=None, la0=0, nla=None, col0=0, ncol=None,
                         amplitudes=None, work_cap_bytes=None, instrument=None):
        """chi2 and the normal equations of the fit of the field vector to observed Stokes profiles at `nodes`
        (include/lsx_hip_fit.h, lsx_hip_fit_field_normal): the field of a column is base_p + sum_n nodes[p][n] basis_p[n] for p of
        B, gammaB, chiB; nnode: the three node counts (0: not fitted); basis [P][Nspace], the rows of B first; nodes [ncol][P];
        base [ncol][3][Nspace] or None; obs, weight [ncol][4][nla][nmu] (weight None: 1).  mus, patterns, la0, nla, col0, ncol as in
        stokes_rays; amplitudes as in stokes_response.  The response never leaves the device.  Read-only.
        instrument: a fit.Instrument over the window's nla wavelengths (include/lsx_hip_fit_instrument.h): obs and weight are
        [ncol][4][nobs][nmu], the Stokes vector and the Jacobian are smeared and sampled on the device before the sums; None: as ever.
        nnode of FOUR counts (include/lsx_hip_stokes_velocity.h, lsx_hip_velocity_fit_normal): the line-of-sight velocity [m/s] is the
        fourth quantity -- its rows last in basis, base [ncol][4][Nspace], .field [ncol][4][Nspace], amplitudes may name 'vlos'
        (100 m/s).  The velocity is then base_3 + its nodes' expansion, never the context's own.
        -> fit.FieldNormal (.chi2, .grad, .hess, .field).  Only the HIP library computes it."""
        from .fit import FieldNormal
        head, keep, ob, wt, nc, P, Ns, nq = self._fit_args('normal', mus, basis, nnode, nodes, obs, weight, base, patterns, la0, nla, col0, ncol,
                                                           work_cap_bytes, instrument)
        amp = self._amplitudes(nq, amplitudes)[1]
        chi2, grad, hess = np.empty(nc), np.empty((nc, P)), np.empty((nc, P, P))
        field = np.empty((nc, nq, Ns))
        self._fit_call('normal', head, (_ptr(amp), ob, wt, _ptr(chi2), _ptr(grad), _ptr(hess), _ptr(field)), nq, instrument)
        del keep
        return FieldNormal(chi2, grad, hess, field)

    def fit_field_chi2(self, mus, basis, nnode, nodes, obs, weight=None, base=None, patterns=None, la0=0, nla=None, col0=0, ncol=None,
                       work_cap_bytes=None, instrument=None):
        """chi2 of the field expanded from `nodes` (lsx_hip_fit_field_chi2): one Stokes pass and the reduction of fit_field_normal --
        its chi2, bit for bit.  Arguments as fit_field_normal.  -> (chi2 [ncol], field [ncol][3][Nspace], or [4] with nnode of four)."""
        head, keep, ob, wt, nc, P, Ns, nq = self._fit_args('chi2', mus, basis, nnode, nodes, obs, weight, base, patterns, la0, nla, col0, ncol,
                                                           work_cap_bytes, instrument)
        chi2, field = np.empty(nc), np.empty((nc, nq, Ns))
        self._fit_call('chi2', head, (ob, wt, _ptr(chi2), _ptr(field)), nq, instrument)
        del keep
        return chi2, field

    def fit_field_step(self, hess, grad, lam, nodes, lo=None, hi=None):
        """The damped step per column (lsx_hip_fit_field_step): (hess + lam diag(hess)) delta = grad by Cholesky on the device,
        trial = clip(nodes + delta, lo, hi), predicted = 2 d.grad - d.hess d for d = trial - nodes.  hess [ncol][P][P], grad, nodes
        [ncol][P], lam [ncol] or a scalar, lo, hi [P] or None (no bound).  -> (trial [ncol][P], predicted [ncol], status [ncol]:
        1 where the system is singular or holds a NaN; then trial = nodes, predicted = 0)."""
        self._need('fit_field', 'lsx_hip_fit_field_step')
        g = f64(np.atleast_2d(np.asarray(grad, dtype=np.float64)))
        nc, P = g.shape
        H = f64(np.asarray(hess, dtype=np.float64).reshape(nc, P, P))
        x = f64(np.broadcast_to(np.asarray(nodes, dtype=np.float64), (nc, P)))
        lm = f64(np.broadcast_to(np.asarray(lam, dtype=np.float64), (nc,)))
        lo_ = f64(np.broadcast_to(np.asarray(-np.inf if lo is None else lo, dtype=np.float64), (P,)))
        hi_ = f64(np.broadcast_to(np.asarray(np.inf if hi is None else hi, dtype=np.float64), (P,)))
        trial, pred, status = np.empty((nc, P)), np.empty(nc), np.empty(nc, dtype=np.int32)
        self.lib.check(self.lib.dll.lsx_hip_fit_field_step(self._h, nc, P, _ptr(H), _ptr(g), _ptr(lm), _ptr(x), _ptr(lo_), _ptr(hi_),
                                                           _ptr(trial), _ptr(pred), _iptr(status)))
        return trial, pred, status

    def _penalty(self, who, penalty, ncol, P, with_target=True):
        """-> (the C struct of a fit.Penalty, what must outlive the call)"""
        self._need('fit_regular', 'lsx_hip_regular_penalty')
        if penalty.nparam != P:
            raise ValueError('%s: the penalty is made for %d node values, the call has %d' % (who, penalty.nparam, P))
        L = f64(penalty.L)
        tg = penalty.targets(ncol) if with_target else None
        return _capi.LsxFitPenalty(penalty.nrow, _ptr(L), _opt(tg)), (L, tg)

    def fit_field_penalty(self, nodes, penalty, chi2, grad=None, hess=None):
        """The penalty of a regularised fit added to what fit_field_normal / fit_field_chi2 returned for `nodes` [ncol][P]
        (include/lsx_hip_fit_regular.h, lsx_hip_regular_penalty): penalty a fit.Penalty; chi2 [ncol], grad [ncol][P], hess [ncol][P][P]
        (both or neither: without them the chi2 of a trial, the bits the full call gives).  The arguments are not changed.
        -> (chi2 + penalty, grad + L^T rho or None, hess + L^T L or None, penalty [ncol]).  Only the HIP library computes it."""
        x = f64(np.atleast_2d(np.asarray(nodes, dtype=np.float64)))
        nc, P = x.shape
        st, keep = self._penalty('fit_field_penalty', penalty, nc, P)
        c = np.array(np.broadcast_to(np.asarray(chi2, dtype=np.float64), (nc,)), dtype=np.float64)
        if (grad is None) != (hess is None):
            raise ValueError('fit_field_penalty: grad and hess go together')
        g = None if grad is None else np.array(np.asarray(grad, dtype=np.float64).reshape(nc, P), dtype=np.float64)
        H = None if hess is None else np.array(np.asarray(hess, dtype=np.float64).reshape(nc, P, P), dtype=np.float64)
        pen = np.empty(nc)
        self.lib.check(self.lib.dll.lsx_hip_regular_penalty(self._h, nc, P, C.byref(st), _ptr(x), _ptr(c), _opt(g), _opt(H), _ptr(pen)))
        del keep
        return c, g, H, pen

    def fit_field_uncertainty(self, hess, basis, nnode, penalty=None, scale=None, ainv=True, field_sigma=True):
        """The uncertainties of the fitted nodes from the DATA's normal equations hess [ncol][P][P] at the solution
        (include/lsx_hip_fit_regular.h, lsx_hip_regular_uncertainty): A = hess + L^T L of the fit.Penalty (None: hess), its inverse by
        Cholesky on the device, cov = scale x ainv hess ainv (the sandwich; without a penalty ainv), sigma = sqrt(diag cov) and the
        standard deviation of the expanded field at every depth from basis [P][Nspace] and nnode (three or four counts, any Nspace).
        scale [ncol], a scalar, or None for 1.  -> fit.FieldUncertainty (.ainv and .field_sigma None if not asked for); a column whose
        system is singular or holds a NaN has status 1 and NaN everywhere.  Only the HIP library computes it."""
        from .fit import FieldUncertainty
        H = f64(np.asarray(hess, dtype=np.float64))
        if H.ndim == 2:
            H = H[None]
        if H.ndim != 3 or H.shape[1] != H.shape[2]:
            raise ValueError('fit_field_uncertainty: hess must be [ncol][P][P]')
        nc, P = H.shape[:2]
        nn = np.ascontiguousarray(np.asarray(nnode).reshape(-1), dtype=np.int32)
        bas = f64(np.atleast_2d(np.asarray(basis, dtype=np.float64)))
        if bas.shape[0] != P:
            raise ValueError('fit_field_uncertainty: basis has %d rows, hess is %d x %d' % (bas.shape[0], P, P))
        Ns = bas.shape[1]
        if penalty is None:
            self._need('fit_regular', 'lsx_hip_regular_uncertainty')
            st, keep = None, None
        else:
            st, keep = self._penalty('fit_field_uncertainty', penalty, nc, P, with_target=False)
        sc = None if scale is None else f64(np.broadcast_to(np.asarray(scale, dtype=np.float64), (nc,)))
        ai = np.empty((nc, P, P)) if ainv else None
        cov, sigma, status = np.empty((nc, P, P)), np.empty((nc, P)), np.empty(nc, dtype=np.int32)
        fs = np.empty((nc, nn.shape[0], Ns)) if field_sigma else None
        self.lib.check(self.lib.dll.lsx_hip_regular_uncertainty(self._h, nc, P, _ptr(H), None if st is None else C.byref(st), _opt(sc),
                                                                nn.shape[0], _iptr(nn), _ptr(bas), Ns, _opt(ai), _ptr(cov), _ptr(sigma),
                                                                _opt(fs), _iptr(status)))
        del keep
        return FieldUncertainty(ai, cov, sigma, fs, status, nn)

    def eos(self, tables, temperature, nHTot):
        """The Wittmann equation of state of the reference's Background (include/lsx_hip_background.h, lsx_hip_eos) for
        temperature, nHTot [ncol][Nspace] (SI; a single column may be 1-D); `tables` is a background.EosTables.
        -> background.EosResult with .pgas, .pe [ncol][Nspace] (dyn cm^-2), .partials [ncol][17][Nspace] and .status (the number of
        witt.pe_pg evaluations per point).  A point that ends at an iteration cap raises LsxError (LSX_ENOCONV).  Does not touch
        the engine's state; any ncol.  Only the HIP library computes it."""
        from .background import EosResult
        self._need('background', 'lsx_hip_eos')
        Ns = self.problem.Nspace
        T = f64(np.asarray(temperature, dtype=np.float64).reshape(-1, Ns))
        nH = f64(nHTot).reshape(-1, Ns)
        if nH.shape != T.shape:
            raise ValueError('temperature and nHTot differ in shape')
        ncol = T.shape[0]
        pgas, pe, part = np.empty((ncol, Ns)), np.empty((ncol, Ns)), np.empty((ncol, 17, Ns))
        status = np.zeros((ncol, Ns), dtype=np.int32)
        ctab, _keep = tables.to_c()
        rc = self.lib.dll.lsx_hip_eos(self._h, C.byref(ctab), ncol, _ptr(T), _ptr(nH), _ptr(pgas), _ptr(pe), _ptr(part), _iptr(status))
        res = EosResult(pgas, pe, part, status)
        if rc == _capi.LSX_ENOCONV:
            err = _capi.LsxError(rc, self.lib.dll.lsx_last_error().decode(errors='replace'))
            err.result = res            # the outputs are written all the same: which points, and how far they got
            raise err
        self.lib.check(rc)
        return res

    def background(self, tables, temperature, nHTot, ne, wavelength=None, col0=0, install=False, read_back=True):
        """Background opacity, emissivity and Thomson scattering coefficient of the reference's Background(atmos, spect)
        (include/lsx_hip_background.h, lsx_hip_background) for temperature, nHTot, ne [ncol][Nspace] (SI; one column may be 1-D).
        wavelength: nm, strictly ascending (None: the problem's own grid).  install=True (own grid only) puts the result into the
        engine as the background of columns [col0, col0 + ncol), which set_columns must have set before.
        -> (chi, eta, sca) with chi, eta [ncol][nla][Nspace] -- what emergent_spectrum takes as bg_chi / bg_eta -- and sca
        [ncol][Nspace]; None when installing with read_back=False.  Only the HIP library computes it."""
        self._need('background', 'lsx_hip_background')
        Ns = self.problem.Nspace
        T = f64(np.asarray(temperature, dtype=np.float64).reshape(-1, Ns))
        nH, el = f64(nHTot).reshape(-1, Ns), f64(ne).reshape(-1, Ns)
        if nH.shape != T.shape or el.shape != T.shape:
            raise ValueError('temperature, nHTot and ne differ in shape')
        ncol = T.shape[0]
        w = None if wavelength is None else _vector(wavelength)
        nla = self.problem.Nspect if w is None else w.shape[0]
        want = read_back or not install
        chi, eta, sca = (np.empty((ncol, nla, Ns)), np.empty((ncol, nla, Ns)), np.empty((ncol, Ns))) if want else (None, None, None)
        ctab, _keep = tables.to_c()
        self.lib.check(self.lib.dll.lsx_hip_background(self._h, C.byref(ctab), int(col0), ncol, _ptr(T), _ptr(nH), _ptr(el), nla, _opt(w),
                                                       _opt(chi), _opt(eta), _opt(sca), 1 if install else 0))
        return (chi, eta, sca) if want else None

    def convert_scales(self, tables, scale, depth_scale, temperature, nHTot, ne=None, logG=2.44, col0=0, install=False, read_back=True):
        """Column mass, geometric height and tau500 of columns given on one of the three, the reference's
        AtmosphereConstructor.convert_scales (include/lsx_hip_scales.h, lsx_hip_convert_scales).  scale: 'geometric',
        'column_mass', 'tau500' or the LSX_SCALE_* values; depth_scale, temperature, nHTot [ncol][Nspace] (SI; one column may be
        1-D); ne likewise, needed for the geometric scale only, as is logG.  install=True puts the resulting height into the engine
        as the height of columns [col0, col0 + ncol), which set_columns must have set before.
        -> atmosphere.Scales with .height, .cmass, .tau_ref, .chi_ref [ncol][Nspace] (chi_ref: the continuous opacity at 500 nm,
        m^-1); None when installing with read_back=False.  Only the HIP library computes it."""
        from .atmosphere import Scales, scale_code
        self._need('scales', 'lsx_hip_convert_scales')
        code = scale_code(scale)
        Ns = self.problem.Nspace
        ds = f64(np.asarray(depth_scale, dtype=np.float64).reshape(-1, Ns))
        T, nH = f64(temperature).reshape(-1, Ns), f64(nHTot).reshape(-1, Ns)
        el = None if ne is None else f64(ne).reshape(-1, Ns)
        if T.shape != ds.shape or nH.shape != ds.shape or (el is not None and el.shape != ds.shape):
            raise ValueError('depth_scale, temperature, nHTot and ne differ in shape')
        if code == _capi.LSX_SCALE_GEOMETRIC and el is None:
            raise ValueError('the geometric scale needs ne')
        ncol = ds.shape[0]
        want = read_back or not install
        out = [np.empty((ncol, Ns)) for _ in range(4)] if want else [None] * 4
        ctab, _keep = tables.to_c()
        self.lib.check(self.lib.dll.lsx_hip_convert_scales(self._h, C.byref(ctab), code, int(col0), ncol, _ptr(ds), _ptr(T), _ptr(nH), _opt(el),
                                                           10**logG, *map(_opt, out), 1 if install else 0))
        return Scales(*out) if want else None

    def eq_pops(self, atoms, abundances, temperature, ne, nHTot, want_nTotal=True):
        """LTE populations of any atoms, active in this engine or not: the reference's RadiativeSet.compute_eq_pops over
        lte_pops(debye=True) (include/lsx_hip_eqpops.h, lsx_hip_eq_pops).  atoms: objects with .E_SI, .g and .stage per level
        (atomdata.AtomData; only the levels are read); abundances: one per atom, relative to hydrogen; temperature, ne, nHTot
        [ncol][Nspace] (SI; one column may be 1-D).
        -> eqpops.EqPops with .nStar (a list per atom of [ncol][Nlevel][Nspace]), .nStar_flat [ncol][sum Nlevel][Nspace] and
        .nTotal [ncol][natoms][Nspace] (None with want_nTotal=False).  For an atom that is active in the engine, nStar holds the
        bits set_atmosphere(lte_pops=True) leaves in LSX_NSTAR.  Does not touch the engine's state; any ncol.  Only the HIP
        library computes it."""
        from .eqpops import EqPops, atoms_to_c
        self._need('eq_pops', 'lsx_hip_eq_pops')
        Ns = self.problem.Nspace
        T = f64(np.asarray(temperature, dtype=np.float64).reshape(-1, Ns))
        el, nH = f64(ne).reshape(-1, Ns), f64(nHTot).reshape(-1, Ns)
        if el.shape != T.shape or nH.shape != T.shape:
            raise ValueError('temperature, ne and nHTot differ in shape')
        ncol = T.shape[0]
        carr, nlev, _keep = atoms_to_c(atoms, abundances)
        nStar = np.empty((ncol, int(sum(nlev)), Ns))
        nTotal = np.empty((ncol, len(nlev), Ns)) if want_nTotal else None
        self.lib.check(self.lib.dll.lsx_hip_eq_pops(self._h, len(nlev), carr, ncol, _ptr(T), _ptr(el), _ptr(nH), _ptr(nStar), _opt(nTotal)))
        return EqPops(nStar, nTotal, nlev)

    def configure_ng(self, order=2, delay=0):
        """Ng acceleration of the populations behind every stat_equil of this engine (include/lsx_hip_ng.h, lsx_hip_ng_configure):
        order 1 or 2, 0 switches it off; `delay` statistical equilibria pass before the first vector is stored.  Also takes an
        NgOptions (or None: off) as `order`.  Every column's history and counters are reset.
        Only the HIP library has it; there is no host version."""
        self._need('ng', 'lsx_hip_ng_configure')
        if order is None:
            order, delay = 0, 0
        elif isinstance(order, NgOptions):
            order, delay = order.order, order.delay
        self.lib.check(self.lib.dll.lsx_hip_ng_configure(self._h, int(order), int(delay)))

    def ng_state(self, col0=0, ncol=None) -> NgState:
        """the Ng state of columns [col0, col0 + ncol) (include/lsx_hip_ng.h, lsx_hip_ng_state)"""
        self._need('ng', 'lsx_hip_ng_state')
        ncol = self._columns(col0, ncol)
        st, ap, rj = (np.zeros(max(ncol, 0), dtype=np.int32) for _ in range(3))
        coef = np.zeros((max(ncol, 0), self.problem.Natoms, 2), dtype=np.float64)
        self.lib.check(self.lib.dll.lsx_hip_ng_state(self._h, int(col0), ncol, _iptr(st), _iptr(ap), _iptr(rj), _ptr(coef)))
        return NgState(st, ap, rj, coef)

    # ---- radiation boundary conditions (include/lsx_hip_boundary.h) ----
    def set_boundary(self, lower='thermalised', upper='zero', I_lower=None, I_upper=None, col0=0, ncol=None):
        """The boundary of columns [col0, col0 + ncol) (lsx_hip_set_boundary): what up-going rays start with at the lower end and
        down-going rays at the upper end.  Kinds: 'zero', 'thermalised', 'given' (boundary.kind_code: strings, enum-like objects
        with .name, the LSX_BOUNDARY_* integers), or a boundary.Boundary as `lower`.  I_lower / I_upper [ncol][Nspect][Nrays], or
        [Nspect][Nrays] for every column of the range: needed exactly where the kind is 'given'.  Engine state: it holds for every
        following formal solution, radiative_rates and radiative_losses until it is set again, set_columns / setup_columns do not
        reset it; emergent_rays, depth_rays and emergent_spectrum refuse a 'given' lower boundary.  An engine on which it has
        never been called has ('thermalised', 'zero').  Only the HIP library has it; there is no host version."""
        from . import boundary as B
        self._need('boundary', 'lsx_hip_set_boundary')
        if isinstance(lower, B.Boundary):
            if I_lower is not None or I_upper is not None or B.kind_code(upper) != B.ZERO:
                raise ValueError('set_boundary: a Boundary brings its own upper kind and arrays')
            lower, upper, I_lower, I_upper = lower.lower, lower.upper, lower.I_lower, lower.I_upper
        lo, up = B.kind_code(lower), B.kind_code(upper)
        ncol = self._columns(col0, ncol)
        shape = (self.problem.Nspect, self.problem.Nrays)
        a_lo = B._array(I_lower, lo, 'lower', shape, max(ncol, 0))
        a_up = B._array(I_upper, up, 'upper', shape, max(ncol, 0))
        self.lib.check(self.lib.dll.lsx_hip_set_boundary(self._h, int(col0), ncol, lo, up, _opt(a_lo), _opt(a_up)))

    def boundary_state(self, col0=0, ncol=None):
        """-> int32 [ncol][2]: the (lower, upper) kinds of columns [col0, col0 + ncol) (lsx_hip_boundary_state; boundary.ZERO,
        .THERMALISED, .GIVEN)"""
        self._need('boundary', 'lsx_hip_boundary_state')
        ncol = self._columns(col0, ncol)
        kinds = np.zeros((max(ncol, 0), 2), dtype=np.int32)
        self.lib.check(self.lib.dll.lsx_hip_boundary_state(self._h, int(col0), ncol, _iptr(kinds)))
        return kinds

    # ---- time-dependent populations (include/lsx_hip_timedep.h) ----
    def time_dep_start(self, dt, n_prev=None, col0=0, ncol=None):
        """Begin a time step of `dt` seconds (a scalar, or one value per column) for columns [col0, col0 + ncol)
        (lsx_hip_time_dep_start).  n_prev [ncol][NLtot][Nspace]: the populations at the start of the step; None: the columns'
        current populations, copied on the device.  The populations themselves are not touched; the range's Ng history is
        discarded.  Only the HIP library has it; there is no host version."""
        self._need('time_dep', 'lsx_hip_time_dep_start')
        ncol = self._columns(col0, ncol)
        if np.ndim(dt) == 0:
            dts = np.full(max(ncol, 0), float(dt), dtype=np.float64)
        else:
            dts = f64(dt, (max(ncol, 0),))
        prev = None if n_prev is None else f64(n_prev, (max(ncol, 0),) + self._shape(_capi.LSX_N))
        self.lib.check(self.lib.dll.lsx_hip_time_dep_start(self._h, int(col0), ncol, _ptr(dts) if dts.size else None, _opt(prev)))

    def time_dep_update(self) -> float:
        """one implicit update of every active column's populations from the last formal solution's Gamma, in the place of
        stat_equil (lsx_hip_time_dep_update) -> max relative population change against the iterate the call started from"""
        self._need('time_dep', 'lsx_hip_time_dep_update')
        v = C.c_double()
        self.lib.check(self.lib.dll.lsx_hip_time_dep_update(self._h, C.byref(v)))
        return v.value

    def time_dep_update_async(self):
        """the same, enqueued: stands where stat_equil_async stands (sync, sync_begin / sync_end, fetch_populations follow as usual)"""
        self._need('time_dep', 'lsx_hip_time_dep_update_async')
        self.lib.check(self.lib.dll.lsx_hip_time_dep_update_async(self._h))

    def time_dep_state(self, col0=0, ncol=None):
        """-> (dt [ncol], n_prev [ncol][NLtot][Nspace]) of columns [col0, col0 + ncol); dt = 0: no step started"""
        self._need('time_dep', 'lsx_hip_time_dep_state')
        ncol = self._columns(col0, ncol)
        dt = np.zeros(max(ncol, 0), dtype=np.float64)
        prev = np.zeros((max(ncol, 0),) + self._shape(_capi.LSX_N), dtype=np.float64)
        self.lib.check(self.lib.dll.lsx_hip_time_dep_state(self._h, int(col0), ncol, _ptr(dt), _ptr(prev)))
        return dt, prev

    def gamma_of_atom(self, G, a):
        """view [ncol][Nl][Nl][Nspace] of atom a inside an LSX_GAMMA array"""
        p = self.problem
        nl = p.Nlevel[a]
        o = p.lev2_off[a]
        return G[:, o:o + nl * nl, :].reshape(G.shape[0], nl, nl, p.Nspace)
