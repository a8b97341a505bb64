"""Drop-in counterpart of Lightspinner's rh_method.Context (rh_method.py:490-745).

    ctx = Context(atmos, spect, eqPops, background)
    dJ = ctx.formal_sol_gamma_matrices()
    dPops = ctx.stat_equil()
    ctx.I, ctx.J, ctx.activeAtoms[0].n / .Gamma / .C / .nStar / .nTotal / .trans[kr].phi ...

The constructor reads the same (duck-typed) attributes the reference's constructor reads from
Lightspinner's Atmosphere / SpectrumConfiguration / AtomicStateTable / Background objects.  Nothing
numerical happens on the host: everything between the atmosphere and the hot path's inputs is
evaluated by the library,

  * setup='native' (chosen by 'auto' when the model objects carry their atomic data: levels with
    E_SI / g / stage, lines with gRad / stark / vdw, collisions that are Omega / CI / CE tables):
    the data go down once (lsx_set_atomic_data) and lsx_set_atmosphere derives vBroad, aDamp, the
    line profiles and the collisional rates on the device (rh_method.py:198-243, 474-487;
    atomic_model.py:66-69, 491-502);
  * setup='methods' (models that only offer the reference's methods): `atom.v_broad`,
    `line.damping` and `collision.compute_rates` are CALLED, as the reference calls them, and
    their results handed over; the profiles are still built on the device
    (lsx_set_line_profiles).

`t.phi`, `t.wphi`, `t.aDamp`, `atom.vBroad` and `atom.C` are read back from the library.  The two
hot calls run on the GPU through the lsx C ABI; there is no CPU fallback (the HIP library must be
built).

Read-back (round 6).  The reference's `ctx.J`, `ctx.I` and `atom.Gamma` are live arrays that every call rewrites in
place; its drivers (test.py:20-29, response_fn.py:11-21) read them once, after the loop.  Here they are fetched from the
device when they are first LOOKED AT: until then a call costs the enqueue, the wait and one 16-byte monitor read-back.
An array that has been handed out once is kept current after every call from then on (its holder may read it, or write it,
at any time: edits are found by comparing with what was last synchronised, as before) -- `readback='eager'` asks for that
from the start.  `atom.n` is the caller's own array (`eqPops[name].pops`, rh_method.py:412-416): stat_equil writes it
in place after every call, always.

Look-ahead (round 6).  test.py:20-29 calls the two verbs in turn; each returns a number the loop's condition needs, so each is a
host round trip with the GPU idle behind it.  stat_equil() here enqueues the NEXT formal solution speculatively behind its own
read-back (lsx_sync_begin_populations / lsx_formal_sol_gamma_speculative, include/lsx.h) before it returns: if the caller's next
call is formal_sol_gamma_matrices() -- and it has not edited n or J in between -- that call only waits for it.  Anything else
(another stat_equil, a look at J / I / Gamma, an edit, update_collisions) takes the speculative call back first
(lsx_discard_formal_sol): every result is what the plain sequence gives, bit for bit (tests/context_cases.py).  `lookahead=False`
switches it off.

Deliberate differences, all outside the numbers the drivers use:
  * `t.Rij` / `t.Rji` are not attributes of the transitions (the reference accumulates them over
    its calls without ever zeroing or reading them, rh_method.py:691-692); accessing them raises
    AttributeError.  `Context.compute_rates()` computes the rates of one formal solution on demand
    from what the context holds, with the reference's form of Rji and the physical one.
  * collisional rates are evaluated when the Context is built and whenever
    `update_collisions()` is called, not on every formal solution (they depend on the
    atmosphere only, rh_method.py:474-487).
"""
from typing import List, Optional

import numpy as np

from . import _capi, atomdata
from . import constants as Const
from .problem import Problem, Transition, ColumnBlock, Engine, RadiativeRates, RadiativeLosses, DepthRays
from .spectrum import continuum_alpha

_KNOWN_COLLISIONS = ('Omega', 'CI', 'CE')


def _same(a, b):
    if a is b:
        return True
    try:
        return bool(a == b)
    except Exception:
        return False


def _contains(seq, item):
    return any(_same(x, item) for x in seq)


def _is_line(trans):
    return hasattr(trans, 'Aji') and hasattr(trans, 'lambda0')


def models_carry_atomic_data(models, atmos) -> bool:
    """can lsx_set_atomic_data be filled from these objects (atomdata.from_models)?"""
    if not all(hasattr(atmos, k) for k in ('ne', 'vturb')):
        return False
    for m in models:
        table = getattr(m, 'atomicTable', None)
        if table is None:
            return False
        try:
            table[m.name].weight, table['H'].weight, table['He'].abundance
        except Exception:
            return False
        if not all(hasattr(l, 'E_SI') and hasattr(l, 'g') and hasattr(l, 'stage') for l in m.levels):
            return False
        if not all(hasattr(l, 'gRad') and hasattr(l, 'stark') for l in m.lines):
            return False
        if not all(type(c).__name__ in _KNOWN_COLLISIONS and hasattr(c, 'temperature') and hasattr(c, 'rates')
                   for c in m.collisions):
            return False
    return True


class ComputationalTransition:
    """rh_method.py:25-288 (state only; uv() lives in the sweep kernel, compute_phi in the set-up kernels)."""

    def __init__(self, trans, compAtom: 'ComputationalAtom', atmos, spect):
        self.transModel = trans
        self.atom = compAtom
        self.wavelength = np.asarray(trans.wavelength, dtype=np.float64)
        self.isLine = _is_line(trans)
        if self.isLine:
            self.Aji, self.Bji, self.Bij, self.lambda0 = float(trans.Aji), float(trans.Bji), float(trans.Bij), float(trans.lambda0)
        else:
            self.alpha = np.asarray(trans.alpha, dtype=np.float64)
        self.i, self.j = int(trans.i), int(trans.j)
        self.Nblue = int(np.searchsorted(spect.wavelength, self.wavelength[0]))       # :122
        self.active = np.zeros(spect.wavelength.shape[0], dtype=bool)                  # :124-127
        for la, s in enumerate(spect.activeSet):
            if _contains(s, trans):
                self.active[la] = True
        self.gij = None
        self._line_index = None          # position among the lines of the transition table
        self._phi_offset = None          # first row of this line in LSX_PHI

    def lt(self, la: int) -> int:
        return la - self.Nblue

    def wlambda(self, la: Optional[int] = None):
        """rh_method.py:157-196: trapezoid weights of the transition's own grid, in Doppler units for a line"""
        lam = self.wavelength
        w = np.empty_like(lam)
        w[0], w[-1] = 0.5 * (lam[1] - lam[0]), 0.5 * (lam[-1] - lam[-2])
        w[1:-1] = 0.5 * (lam[2:] - lam[:-2])
        if self.isLine:
            w *= Const.CLight / self.lambda0
        return w if la is None else w[la]

    # -- read back from the library ------------------------------------------------------
    def _need_line(self):
        if not self.isLine:
            raise AttributeError('a continuum has no line profile')
        return self.atom._context

    @property
    def phi(self):
        """[Nlambda][Nrays][2][Nspace] (rh_method.py:224)"""
        ctx = self._need_line()
        p = ctx.problem
        phi = ctx._profiles()[0][self._phi_offset:self._phi_offset + self.wavelength.shape[0]]
        if p.phi_compact:
            phi = np.broadcast_to(phi[:, None, None, :], (phi.shape[0], p.Nrays, 2, p.Nspace))
        return phi

    @property
    def wphi(self):
        return self._need_line()._profiles()[1][self._line_index]

    @property
    def aDamp(self):
        return self._need_line()._damping()[self._line_index]


class ComputationalAtom:
    """rh_method.py:290-487."""

    def __init__(self, atom, atmos, spect, eqPops):
        self.atomicModel = atom
        self.atomicTable = getattr(eqPops, 'atomicTable', None)
        self.spect = spect
        self.atmos = atmos
        self.pops = eqPops[atom.name]
        self.hPops = eqPops['H']
        self.nTotal = self.pops.nTotal
        self.trans: List[ComputationalTransition] = []
        for l in atom.lines:                                   # lines first, then continua, :399-405
            if _contains(spect.transitions, l):
                self.trans.append(ComputationalTransition(l, self, atmos, spect))
        for c in atom.continua:
            if _contains(spect.transitions, c):
                self.trans.append(ComputationalTransition(c, self, atmos, spect))
        Nlevel = len(atom.levels)
        self.Nlevel = Nlevel
        self.Ntrans = len(self.trans)
        self._Gamma = np.zeros((Nlevel, Nlevel, atmos.Nspace))
        self.nStar = self.pops.nStar
        if self.pops.pops is not None:                         # warm start, :412-416
            self.n = self.pops.pops
        else:
            self.n = np.copy(self.nStar)
            self.pops.pops = self.n
        self._context = None
        self._index = None

    @property
    def Gamma(self):
        """[Nlevel][Nlevel][Nspace], rh_method.py:587-590, 698-703 (fetched when first looked at, kept current from then on)"""
        ctx = self._context
        if ctx is None:
            return self._Gamma
        return ctx._lazy_out('Gamma')[self._index]

    @property
    def vBroad(self):
        return self._context._broadening()[self._index]

    @property
    def C(self):
        """[Nlevel][Nlevel][Nspace] collisional rates as the library holds them (rh_method.py:474-487)"""
        ctx = self._context
        return ctx._engine.gamma_of_atom(ctx._engine.get(_capi.LSX_C), self._index)[0]


class Context:
    """rh_method.py:490-745 on the GPU."""

    def __init__(self, atmos, spect, eqPops, background, device: int = 0, stream=None, lib=None, setup: str = 'auto',
                 formal_solver: str = 'linear', readback: str = 'lazy', lookahead: Optional[bool] = None, *, ng=None,
                 boundary=None):
        # boundary (include/lsx_hip_boundary.h): None -- the reference's hard-wired pair (thermalised below, zero above): the
        # reference ignores atmos.lowerBc / upperBc, and a drop-in gives the reference's numbers for the reference's inputs; no call
        # to the setter is made.  'atmos': the kinds the atmosphere carries.  A boundary.Boundary: applied as given.
        self.atmos = atmos
        self.atmos.nondimensionalise()
        self.spect = spect
        self.background = background
        self.eqPops = eqPops
        self.activeAtoms: List[ComputationalAtom] = [ComputationalAtom(a, atmos, spect, eqPops)
                                                     for a in spect.radSet.activeAtoms]
        Nspect, Nspace, Nrays = spect.wavelength.shape[0], atmos.Nspace, atmos.Nrays
        if readback not in ('lazy', 'eager'):
            raise ValueError("readback must be 'lazy' or 'eager'")
        # the result arrays (one object each for the life of the context, rewritten in place like the reference's), whether the
        # device holds something newer (`_stale`), and whether somebody outside holds them (`_handed`: kept current and checked for edits)
        self._host = {'J': np.zeros((Nspect, Nspace)), 'I': np.zeros((Nspect, Nrays)),
                      'Gamma': [a._Gamma for a in self.activeAtoms]}
        self._stale = {'J': False, 'I': False, 'Gamma': False}
        self._handed = {k: readback == 'eager' for k in self._host}
        self._J_synced = None
        models = [a.atomicModel for a in self.activeAtoms]
        if setup == 'auto':
            setup = 'native' if models_carry_atomic_data(models, atmos) else 'methods'
        if setup not in ('native', 'methods'):
            raise ValueError("setup must be 'auto', 'native' or 'methods'")
        self.setup = setup

        # ---- flatten to the lsx problem description --------------------------------------
        trans, active = [], []
        nline = off = 0
        for a, atom in enumerate(self.activeAtoms):
            atom._context, atom._index = self, a
            for t in atom.trans:
                tr = Transition(atom=a, is_line=t.isLine, i=t.i, j=t.j, Nblue=t.Nblue, Nlambda=t.wavelength.shape[0])
                if t.isLine:
                    tr.Aji, tr.Bji, tr.Bij, tr.lambda0 = t.Aji, t.Bji, t.Bij, t.lambda0
                    t._line_index, t._phi_offset = nline, off
                    nline += 1
                    off += t.wavelength.shape[0]
                else:
                    tr.alpha = t.alpha
                trans.append(tr)
                active.append(t.active)
        sca = np.asarray(background.sca, dtype=np.float64)
        sca_per_lambda = not (sca.ndim == 2 and np.all(sca == sca[0:1]))
        phi_compact = bool(np.all(np.asarray(atmos.vlos) == 0.0))
        self.problem = Problem(Nspace=Nspace, wavelength=np.asarray(spect.wavelength), muz=atmos.muz, wmu=atmos.wmu,
                               Nlevel=[a.Nlevel for a in self.activeAtoms], trans=trans,
                               active=np.array(active, dtype=bool).reshape(len(trans), Nspect),
                               sca_per_lambda=sca_per_lambda, phi_compact=phi_compact,
                               atom_names=[a.atomicModel.name for a in self.activeAtoms])
        self._engine = Engine(self.problem, 1, device=device, stream=stream, lib=lib)
        if formal_solver != 'linear':          # 'parabolic': the monotonic piecewise-parabolic rule (include/lsx.h, N4; not in the reference)
            self._engine.set_formal_solver(formal_solver)
        if ng is not None and ng.order:         # problem.NgOptions: Ng acceleration behind every stat_equil (include/lsx_hip_ng.h)
            self._engine.configure_ng(ng)
        if boundary is not None:
            from .boundary import Boundary
            if isinstance(boundary, str):
                if boundary != 'atmos':
                    raise ValueError("boundary must be None, 'atmos' or a boundary.Boundary")
                boundary = Boundary.from_atmos(atmos)
            elif not isinstance(boundary, Boundary):
                raise ValueError("boundary must be None, 'atmos' or a boundary.Boundary")
            self._engine.set_boundary(boundary)
        self.boundary = boundary
        self._cache = {}
        if setup == 'native':
            in_table = lambda m, l: _contains(spect.transitions, l)
            self._engine.set_atomic_data(atomdata.from_models(models, line_filter=in_table))
        self._upload()
        # stat_equil enqueues the next formal solution ahead where the library says that pays (one launch chain on one stream)
        self._lookahead = self._engine.prefers_lookahead() if lookahead is None else bool(lookahead)
        self._spec = False               # a speculative formal solution is enqueued and has not been accepted or taken back
        self._td_step = None             # (prevTimePops, dt) of the time step time_dep_update has started
        self._n_synced = [np.array(a.n, dtype=np.float64) for a in self.activeAtoms]
        if self._handed['J']:
            self._J_synced = self._host['J'].copy()

    # -- the live result arrays ------------------------------------------------------------
    def _cancel_lookahead(self):
        """take the speculative formal solution back: the library's results are the last ACCEPTED call's again"""
        if self._spec:
            self._engine.discard_formal_sol()
            self._spec = False

    def _fetch(self, what):
        self._cancel_lookahead()
        eng = self._engine
        if what == 'J':
            self._host['J'][...] = eng.get(_capi.LSX_J)[0]
            if self._handed['J']:
                self._J_synced = self._host['J'].copy()
        elif what == 'I':
            self._host['I'][...] = eng.get(_capi.LSX_I)[0]
        else:
            G = eng.get(_capi.LSX_GAMMA)
            for a, arr in enumerate(self._host['Gamma']):
                arr[...] = eng.gamma_of_atom(G, a)[0]
        self._stale[what] = False

    def _lazy_out(self, what):
        """the array, current; from now on somebody outside may hold it"""
        if self._stale[what]:
            self._fetch(what)
        if not self._handed[what]:
            self._handed[what] = True
            if what == 'J':
                self._J_synced = self._host['J'].copy()
        return self._host[what]

    @property
    def J(self):
        """[Nspect][Nspace] mean intensity, rh_method.py:562, 640"""
        return self._lazy_out('J')

    @J.setter
    def J(self, value):
        self._lazy_out('J')[...] = value          # found by the next call's comparison and sent down

    @property
    def I(self):
        """[Nspect][Nrays] emergent intensity, rh_method.py:563, 638"""
        return self._lazy_out('I')

    def _results_changed(self, names):
        """a call has rewritten these on the device: refresh the ones somebody holds, mark the others"""
        for k in names:
            if self._handed[k]:
                self._fetch(k)
            else:
                self._stale[k] = True

    # -- packing -------------------------------------------------------------------------
    def _cat_n(self):
        return np.concatenate([np.asarray(a.n, dtype=np.float64) for a in self.activeAtoms], axis=0)

    def _row(self, x):
        return np.asarray(x, dtype=np.float64)[None]

    def _upload(self):
        """atmosphere, populations, background -> library; then the set-up chain (native) or the models' own numbers
        (methods) -> vBroad, aDamp, profiles, collisional rates"""
        p, atmos, bg = self.problem, self.atmos, self.background
        sca = np.asarray(bg.sca, dtype=np.float64)
        sca = sca if p.sca_per_lambda else (sca[0] if sca.ndim == 2 else sca)
        native = self.setup == 'native'
        if native:
            C = np.zeros((p.NL2tot, p.Nspace))
        else:
            C = np.concatenate([self._model_collisions(a).reshape(-1, p.Nspace) for a in self.activeAtoms], axis=0)
        nTotal = np.stack([np.asarray(a.nTotal, dtype=np.float64) for a in self.activeAtoms])
        block = ColumnBlock(
            height=self._row(atmos.height), temperature=self._row(atmos.temperature),
            nStar=np.concatenate([np.asarray(a.nStar) for a in self.activeAtoms], axis=0)[None], nTotal=nTotal[None],
            n=self._cat_n()[None], C=C[None], bg_chi=self._row(bg.chi), bg_eta=self._row(bg.eta), bg_sca=sca[None],
            phi=None, wphi=None)
        self._engine.set_columns(0, block)
        vlos = None if p.phi_compact else self._row(atmos.vlos)
        self._cache = {}
        if native:
            hGround = self.activeAtoms[0].hPops.n[0] if self.activeAtoms else np.zeros(p.Nspace)
            self._engine.set_atmosphere(0, self._row(atmos.temperature), self._row(atmos.ne), self._row(atmos.vturb),
                                        self._row(hGround), nTotal[None], vlos=vlos, lte_pops=False)
        elif p.Nlines:
            vB = np.stack([np.asarray(a.atomicModel.v_broad(atmos), dtype=np.float64) for a in self.activeAtoms])
            aD = np.stack([np.asarray(t.transModel.damping(atmos, vB[a], atom.hPops.n[0])[0], dtype=np.float64)
                           for a, atom in enumerate(self.activeAtoms) for t in atom.trans if t.isLine])
            self._engine.set_line_profiles(0, aD[None], vB[None], vlos)
            self._cache.update(vBroad=vB, aDamp=aD)

    def _model_collisions(self, atom):
        """rh_method.py:474-487 through the models' own compute_rates"""
        C = np.zeros((atom.Nlevel, atom.Nlevel, self.problem.Nspace))
        for col in atom.atomicModel.collisions:
            col.compute_rates(self.atmos, atom.nStar, C)
        C[C < 0.0] = 0.0
        return C

    # -- read-back of what the library derived ---------------------------------------------
    def _profiles(self):
        if 'phi' not in self._cache:
            self._cache['phi'] = (self._engine.get(_capi.LSX_PHI)[0], self._engine.get(_capi.LSX_WPHI)[0])
        return self._cache['phi']

    def _damping(self):
        if 'aDamp' not in self._cache:
            self._cache['aDamp'] = self._engine.get(_capi.LSX_ADAMP)[0]
        return self._cache['aDamp']

    def _broadening(self):
        if 'vBroad' not in self._cache:
            self._cache['vBroad'] = self._engine.get(_capi.LSX_VBROAD)[0]
        return self._cache['vBroad']

    def update_collisions(self):
        """re-derive everything that depends on the atmosphere alone (the reference recomputes the collisional rates
        on every formal solution, rh_method.py:589) and keep J"""
        self._cancel_lookahead()
        if self._stale['J']:
            self._fetch('J')
        J = self._host['J'].copy()
        self._upload()
        self._engine.set(_capi.LSX_J, J[None])

    def _host_edits(self):
        """the reference's arrays are live numpy objects the caller may edit between calls.  The populations are the caller's own
        arrays (eqPops[...].pops): compared on every call (a few kB).  J can only have been edited if it has been handed out.
        -> (n edited, J edited)"""
        n_ed = any(not np.array_equal(a.n, s) for a, s in zip(self.activeAtoms, self._n_synced))
        J_ed = self._handed['J'] and not self._stale['J'] and not np.array_equal(self._host['J'], self._J_synced)
        return n_ed, J_ed

    def _push_host_edits(self, edits=None):
        n_ed, J_ed = self._host_edits() if edits is None else edits
        if n_ed:
            self._engine.set(_capi.LSX_N, self._cat_n()[None])
            self._n_synced = [np.array(a.n, dtype=np.float64) for a in self.activeAtoms]
        if J_ed:
            self._engine.set(_capi.LSX_J, self._host['J'][None])
            self._J_synced = self._host['J'].copy()

    # -- the two verbs ---------------------------------------------------------------------
    def formal_sol_gamma_matrices(self) -> float:
        """rh_method.py:565-708 -> max relative change of J"""
        edits = self._host_edits()
        if self._spec and not any(edits):
            # the formal solution stat_equil enqueued ahead IS this call: wait for it
            self._spec = False
            dJ = self._engine.sync()[0]
        else:
            self._cancel_lookahead()
            self._push_host_edits(edits)
            dJ = self._engine.formal_sol_gamma()
        self._results_changed(('J', 'I', 'Gamma'))
        return dJ

    def compute_rays(self, mus=1.0, wavelengths=None, background=None):
        """Emergent intensity at arbitrary viewing angles: what the reference computes with a Context on atmos.rays(mus)
        (atmosphere.py:386-393) that holds these populations and this J, after one formal_sol_gamma_matrices().  A float
        gives [Nspect], a sequence [Nspect][nmu].  Nothing of the context changes: ctx.I stays the quadrature's.
        wavelengths: None for the context's own grid; otherwise any strictly ascending wavelengths [nm] -- an instrument's sampling of
        a line, a finer grid, continuum points outside the grid: what the reference computes on
        compute_wavelength_grid(extraWavelengths=wavelengths) with these populations (include/lsx_hip_spectrum.h); J is interpolated
        linearly between the grid's points and held constant outside.  -> [nla] or [nla][nmu].
        background: with `wavelengths`, an object with .chi, .eta (and .sca) of [nla][Nspace] at those wavelengths, e.g. the
        reference's Background(atmos, SimpleNamespace(wavelength=wavelengths)); None: the context's own background is interpolated
        like J, an approximation between grid points."""
        self._cancel_lookahead()                  # (the library's J is the last accepted call's again)
        self._push_host_edits()
        scalar = np.ndim(mus) == 0
        mu = np.atleast_1d(np.asarray(mus, dtype=np.float64))
        if wavelengths is None:
            if background is not None:
                raise ValueError('compute_rays: a background is taken with wavelengths only')
            out = self._engine.emergent_rays(mu)[0]
            return out[:, 0] if scalar else out
        w = np.atleast_1d(np.asarray(wavelengths, dtype=np.float64)).reshape(-1)
        conts = [t for a in self.activeAtoms for t in a.trans if not t.isLine]
        alpha = (np.stack([np.asarray(continuum_alpha(t.transModel, w, lib=self._engine.lib), dtype=np.float64) for t in conts])
                 if conts else None)
        bg = {}
        if background is not None:
            bg = dict(bg_chi=np.asarray(background.chi, dtype=np.float64)[None], bg_eta=np.asarray(background.eta, dtype=np.float64)[None])
            if self.problem.sca_per_lambda:
                bg['bg_sca'] = np.asarray(background.sca, dtype=np.float64)[None]
        out = self._engine.emergent_spectrum(mu, w, alpha=alpha, **bg)[0]
        return out[:, 0] if scalar else out

    def compute_depth_rays(self, mus=1.0, la0=0, nla=None, transition=None):
        """WHERE the emergent intensity forms: opacity chi, source function S, optical depth tau, up-going intensity I and the
        contribution function chi S exp(-tau) / mu at every depth along the rays with direction cosines `mus`, and the height at
        which tau = 1, for the wavelengths [la0, la0 + nla) of spect.wavelength -- what the reference builds inside a formal
        solution on atmos.rays(mus) and throws away (rh_method.py:601-638).  transition: one of the context's transitions (the
        object, or its place in [t for atom in activeAtoms for t in atom.trans]) selects that transition's own window instead.
        -> an object with .chi .S .tau .I .contrib, each [nmu][Nspace][nla] ([Nspace][nla] for a float mu), .z_tau1 [nmu][nla]
        ([nla]), .mus, .la0.  Nothing of the context changes."""
        self._cancel_lookahead()                  # (the library's J is the last accepted call's again)
        self._push_host_edits()
        if transition is not None:
            if isinstance(transition, (int, np.integer)):
                transition = [t for a in self.activeAtoms for t in a.trans][int(transition)]
            la0, nla = int(transition.Nblue), int(transition.wavelength.shape[0])
        scalar = np.ndim(mus) == 0
        r = self._engine.depth_rays(np.atleast_1d(np.asarray(mus, dtype=np.float64)), la0=la0, nla=nla)
        pick = (lambda a: a[0, 0]) if scalar else (lambda a: a[0])
        return DepthRays(r.mus, r.la0, **{w: pick(getattr(r, w)) for w in DepthRays.FIELDS})

    def compute_stokes(self, mus, B, gammaB, chiB, transition=None, la0=0, nla=None, instrument=None, vlos=None):
        """Emergent Stokes spectra I, Q, U, V in a magnetic field (Zeeman effect) by the field-free method: these populations and
        this J, one polarised formal solution (DELO-linear) along the rays with direction cosines `mus`.  B [T], gammaB, chiB [rad]:
        [Nspace] or scalars -- strength, inclination against the vertical, azimuth; +Q lies along the projection of the vertical
        on the sky, a field pointing at the observer gives V > 0 on the blue flank of an absorption line (include/lsx_hip_stokes.h).
        The Zeeman patterns come from the context's own line models (zeeman.zeeman_components: gLandeEff, or LS coupling from the
        levels' J, L, S); a line without either stays unpolarised.  transition: one of the context's transitions (the object, or its
        place in [t for atom in activeAtoms for t in atom.trans]) selects that transition's own window, as in compute_depth_rays.
        instrument: a fit.Instrument over the window's wavelengths: the spectra as it sees them, [nobs][nmu] (Engine.apply_instrument).
        vlos [m/s], a scalar or [Nspace]: the line-of-sight velocity of this call in the place of the atmosphere's, with its sign
        convention (include/lsx_hip_stokes_velocity.h).  Populations and J stay the context's: they do not follow it.
        -> an object with .I .Q .U .V, each [nla][nmu] ([nla] for a float mu), .mus, .la0.  Nothing of the context changes."""
        from . import zeeman
        from .problem import StokesRays
        self._cancel_lookahead()                  # (the library's J is the last accepted call's again)
        self._push_host_edits()
        if transition is not None:
            if isinstance(transition, (int, np.integer)):
                transition = [t for a in self.activeAtoms for t in a.trans][int(transition)]
            la0, nla = int(transition.Nblue), int(transition.wavelength.shape[0])
        patterns = [zeeman.zeeman_components(t.transModel) for a in self.activeAtoms for t in a.trans if t.isLine]
        scalar = np.ndim(mus) == 0
        r = self._engine.stokes_rays(np.atleast_1d(np.asarray(mus, dtype=np.float64)), B, gammaB, chiB, patterns=patterns, la0=la0, nla=nla,
                                     vlos=vlos)
        pick = (lambda a: a[0, :, 0]) if scalar else (lambda a: a[0])
        if instrument is not None:
            seen = self._engine.apply_instrument(np.stack([getattr(r, w) for w in StokesRays.FIELDS], axis=1), instrument)
            return StokesRays(r.mus, r.la0, *(pick(seen[:, i]) for i in range(4)))
        return StokesRays(r.mus, r.la0, *(pick(getattr(r, w)) for w in StokesRays.FIELDS))

    def compute_stokes_response(self, mus, B, gammaB, chiB, transition=None, la0=0, nla=None, parameters=('B', 'gammaB', 'chiB'),
                                amplitudes=None, ks=None, vlos=None):
        """Response functions of the emergent Stokes vector of compute_stokes to the field strength, inclination and azimuth at every
        depth: RF_p[k] = (S(p_k + a_p / 2) - S(p_k - a_p / 2)) / a_p, per tesla resp. per radian.  In the field-free method this
        is the change of one polarised formal solution: no NLTE solve (include/lsx_hip_stokes_response.h).  mus, B, gammaB, chiB,
        transition, la0, nla and the Zeeman patterns as in compute_stokes; parameters: some of 'B', 'gammaB', 'chiB'; amplitudes:
        a dict from those names to a_p (default 1e-3 T, 1e-3 rad); ks: the depths (None: all).  vlos as in compute_stokes; 'vlos'
        may then be among the parameters (per m/s, default amplitude 100 m/s), and where it is requested without a velocity the
        atmosphere's own vlos is the velocity of the call.
        -> an object with .rf[name], each [4][nla][nk][nmu] ([4][nla][nk] for a float mu), .stokes (what compute_stokes returns),
        .ks, .mus, .la0, .amplitudes.  Nothing of the context changes."""
        from . import zeeman
        from .problem import StokesRays, StokesResponse
        self._cancel_lookahead()                  # (the library's J is the last accepted call's again)
        self._push_host_edits()
        if transition is not None:
            if isinstance(transition, (int, np.integer)):
                transition = [t for a in self.activeAtoms for t in a.trans][int(transition)]
            la0, nla = int(transition.Nblue), int(transition.wavelength.shape[0])
        patterns = [zeeman.zeeman_components(t.transModel) for a in self.activeAtoms for t in a.trans if t.isLine]
        scalar = np.ndim(mus) == 0
        if vlos is None and 'vlos' in ([parameters] if isinstance(parameters, str) else list(parameters)):
            vlos = self._atmos_vlos()
        r = self._engine.stokes_response(np.atleast_1d(np.asarray(mus, dtype=np.float64)), B, gammaB, chiB, patterns=patterns, la0=la0,
                                         nla=nla, parameters=parameters, amplitudes=amplitudes, ks=ks, vlos=vlos)
        pick = (lambda a: a[0, :, 0]) if scalar else (lambda a: a[0])
        stokes = StokesRays(r.mus, r.la0, *(pick(getattr(r.stokes, w)) for w in StokesRays.FIELDS))
        return StokesResponse({w: (a[0, ..., 0] if scalar else a[0]) for w, a in r.rf.items()}, stokes, r.ks, r.mus, r.la0, r.amplitudes)

    def _atmos_vlos(self):
        """the atmosphere's line-of-sight velocity [Nspace] (zeros where it has none)"""
        Ns = self._engine.problem.Nspace
        v = getattr(self.atmos, 'vlos', None)
        return np.zeros(Ns) if v is None else np.broadcast_to(np.asarray(v, dtype=np.float64), (Ns,)).copy()

    def fit_field(self, mus, obs, transition=None, basis=None, start=None, nnode=None, weight=None, base=None, la0=0, nla=None,
                  amplitudes=None, instrument=None, **loop):
        """Fit the magnetic field vector to observed Stokes profiles obs [4][nla][nmu] ([4][nla] for a float mu) by the field-free
        method: these populations and this J, Levenberg-Marquardt on the node values of field_p = base_p + sum_n x[p][n] basis_p[n]
        (drivers.fit_field_columns on the context's engine; include/lsx_hip_fit.h).  basis [P][Nspace] with nnode = the node counts of
        (B, gammaB, chiB), or a dict from those names to row sets (fit.hat_basis makes them); start: the first node values [P];
        weight as obs or None; base [3][Nspace] or None; mus, transition, la0, nla and the Zeeman patterns as in compute_stokes;
        amplitudes as in compute_stokes_response; instrument: a fit.Instrument over the window's wavelengths, then obs and weight are
        [4][nobs][nmu]; **loop: lo, hi, lambda0, factor, lambda_min, lambda_max, tol, max_iter, log, and penalty (a fit.Penalty:
        the regularised fit), uncertainty (True: .uncertainty holds the nodes' covariance and the field's error band) and scale
        (None, a number or 'reduced'), as drivers.fit_field_columns takes them (include/lsx_hip_fit_regular.h).
        With 'vlos' rows in the basis dict (or nnode of four counts) the line-of-sight velocity [m/s] is fitted with the field
        (include/lsx_hip_stokes_velocity.h): vlos = base_3 + its nodes' expansion, base [4][Nspace]; base None: zeros for the field and
        the atmosphere's vlos for the velocity.  Populations and J do not follow the velocity.  .field has 4 rows.
        -> fit.FieldFit without the column axis.  Nothing of the context changes."""
        from . import zeeman
        from .drivers import fit_field_columns
        from .fit import FieldFit, FieldUncertainty, stack_basis
        self._cancel_lookahead()                  # (the library's J is the last accepted call's again)
        self._push_host_edits()
        if transition is not None:
            if isinstance(transition, (int, np.integer)):
                transition = [t for a in self.activeAtoms for t in a.trans][int(transition)]
            la0, nla = int(transition.Nblue), int(transition.wavelength.shape[0])
        if isinstance(basis, dict):
            basis, nnode = stack_basis(**basis)
        if basis is None or start is None or nnode is None:
            raise ValueError('fit_field: basis (with nnode, or as a dict per parameter) and start are needed')
        if len(nnode) == 4 and base is None:
            base = np.zeros((4, self._engine.problem.Nspace))
            base[3] = self._atmos_vlos()
        patterns = [zeeman.zeeman_components(t.transModel) for a in self.activeAtoms for t in a.trans if t.isLine]
        mu = np.atleast_1d(np.asarray(mus, dtype=np.float64))
        nla_ = self._engine.problem.Nspect - int(la0) if nla is None else int(nla)
        npix = nla_ if instrument is None else instrument.nobs
        shape = (1, 4, npix, mu.shape[0])
        if instrument is not None:
            loop['instrument'] = instrument
        r = fit_field_columns(self._engine, np.asarray(obs, dtype=np.float64).reshape(shape), mu, basis, np.asarray(start)[None, :], nnode,
                              weight=None if weight is None else np.broadcast_to(np.asarray(weight, dtype=np.float64).reshape(
                                  (1, 4, npix, -1) if np.ndim(weight) else ()), shape),
                              base=None if base is None else np.asarray(base, dtype=np.float64)[None], patterns=patterns, la0=la0, nla=nla_,
                              amplitudes=amplitudes, **loop)
        u = r.uncertainty
        if u is not None:
            u = FieldUncertainty(None if u.ainv is None else u.ainv[0], u.cov[0], u.sigma[0],
                                 None if u.field_sigma is None else u.field_sigma[0], u.status[0], u.nnode)
        return FieldFit(r.nodes[0], r.field[0], r.chi2[0], r.history[:, 0], r.lam[0], r.iterations[0], r.status[0], r.nnode,
                        penalty=r.penalty[0], chi2_data=r.chi2_data[0], uncertainty=u, dof=lambda: None if r.dof is None else r.dof[0])

    def compute_rates(self):
        """Radiative rates of every transition (rh_method.py:691-692) as ONE formal solution gives them from these populations and
        this J: -> an object with .Rij, .Rji, .Rji_ref, each [Ntrans][Nspace] in the order of `.transitions`
        ([t for atom in activeAtoms for t in atom.trans]), and .net() = n_j Rji - n_i Rij, the net radiative bracket.
        Rji is the physical downward rate (Vji in the stimulated term); Rji_ref is the reference's line 692 (Vij there), which on a
        fresh context is the reference's t.Rji after its first call.  The reference accumulates over its calls; this does not.
        Nothing of the context changes."""
        self._cancel_lookahead()                  # (the library's J is the last accepted call's again)
        self._push_host_edits()
        r = self._engine.radiative_rates()
        trans = [t for a in self.activeAtoms for t in a.trans]
        pops = [(np.array(t.atom.n[t.i], dtype=np.float64), np.array(t.atom.n[t.j], dtype=np.float64)) for t in trans]
        return RadiativeRates(r.Rij[0], r.Rji[0], r.Rji_ref[0], transitions=trans, populations=pops)

    def compute_losses(self, wavelength_band=None, what=('F', 'Q', 'Qt')):
        """What the radiation does to the gas, as ONE formal solution gives it from these populations and this J
        (include/lsx_hip_losses.h): -> an object with .F [Nspace], the radiative flux in W m^-2 (positive towards the observer),
        .Q [Nspace], the net radiative cooling in W m^-3 (positive: the gas loses energy; dF/dz = Q), .Qt [Ntrans][Nspace], the
        cooling of each transition in the order of `.transitions` ([t for atom in activeAtoms for t in atom.trans]) with
        .total() and .by_transition(names), and .wnu, the frequency weights used.  wavelength_band: (lo, hi) in nm restricts F and
        Q to the wavelengths lo <= lambda <= hi of spect.wavelength (the trapezoid weights, zeroed outside); Qt is summed over
        each transition's own wavelengths either way.  `what` may add 'H' and 'D', the monochromatic sums [Nspect][Nspace].
        F and Q are only as bolometric as spect.wavelength is.  Nothing of the context changes."""
        self._cancel_lookahead()                  # (the library's J is the last accepted call's again)
        self._push_host_edits()
        wnu = None
        if wavelength_band is not None:
            lo, hi = (float(x) for x in wavelength_band)
            lam = np.asarray(self.spect.wavelength, dtype=np.float64)
            wnu = np.where((lam >= lo) & (lam <= hi), self._engine.frequency_weights(), 0.0)
        r = self._engine.radiative_losses(wnu=wnu, what=what)
        trans = [t for a in self.activeAtoms for t in a.trans]
        return RadiativeLosses(r.wnu, transitions=trans,
                               **{w: getattr(r, w)[0] for w in RadiativeLosses.FIELDS if getattr(r, w) is not None})

    def stat_equil(self) -> float:
        """rh_method.py:710-745 -> max relative population change; populations are written back IN
        PLACE into the arrays that alias eqPops[...].pops (rh_method.py:412-416, response_fn.py:62)"""
        return self._population_update(self._engine.stat_equil_async, self._engine.stat_equil)

    def time_dep_update(self, dt, prevTimePops=None):
        """One implicit update of the populations over a time step of `dt` seconds from the last formal solution's Gamma, in the
        place of stat_equil (include/lsx_hip_timedep.h) -> (dPops, prevTimePops).  The first call of a step, with
        prevTimePops=None, starts the step from the current populations and returns them (a list with one [Nlevel][Nspace] array
        per active atom, copies); later calls of the step pass that object back and iterate on.  Any other object -- or another
        dt -- starts a step from the populations it holds.  The populations are written back in place like stat_equil's."""
        self._cancel_lookahead()
        self._push_host_edits()
        eng = self._engine
        if prevTimePops is None:
            prevTimePops = [np.array(a.n, dtype=np.float64) for a in self.activeAtoms]
            eng.time_dep_start(float(dt))
            self._td_step = (prevTimePops, float(dt))
        elif self._td_step is None or prevTimePops is not self._td_step[0] or float(dt) != self._td_step[1]:
            prev = np.concatenate([np.asarray(p, dtype=np.float64) for p in prevTimePops], axis=0)
            eng.time_dep_start(float(dt), n_prev=prev[None])
            self._td_step = (prevTimePops, float(dt))
        return self._population_update(eng.time_dep_update_async, eng.time_dep_update), prevTimePops

    def _population_update(self, enqueue, blocking) -> float:
        """a call that rewrites the populations from the last formal solution's Gamma, and their way back into the callers' arrays"""
        self._cancel_lookahead()                  # (a second stat_equil in a row works on the same Gamma, as in the reference)
        self._push_host_edits()
        eng = self._engine
        if self._lookahead:
            enqueue()
            eng.sync_begin(populations=True)      # monitors + n, read back behind the solve ...
            try:
                eng.formal_sol_gamma_speculative()    # ... and the next iteration's formal solution behind the read-back
                self._spec = True
            except _capi.LsxError:
                self._spec = False
            try:
                dPops = eng.sync_end()[1]
            except _capi.LsxError:
                self._cancel_lookahead()          # (a singular system, rh_method.py:739: nothing is built on it)
                raise
            n = eng.fetch_populations()[0]
        else:
            dPops = blocking()
            n = eng.get(_capi.LSX_N)[0]
        off = 0
        for a, atom in enumerate(self.activeAtoms):
            atom.n[...] = n[off:off + atom.Nlevel]
            self._n_synced[a] = n[off:off + atom.Nlevel]
            off += atom.Nlevel
        return dPops

    def close(self):
        self._spec = False
        self._engine.close()
