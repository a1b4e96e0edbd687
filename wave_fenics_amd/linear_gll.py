"""LinearGLLOpt -- the explicit RK4 wave model of common/LinearGLL.hpp:37-288 on
device vectors, calling libwavehip for every operator and vector kernel.

Same constructor arguments, init(), f0(), f1(), rk4() as the reference.  The
mesh/meshtags pair of the reference is replaced by a FunctionSpace plus the
two tagged boundary dof sets (tag 1 = Neumann source Gamma_1, tag 2 = first-order
absorbing Gamma_2) with their collocated facet masses; the FFCx form
L = c0^2 (g v ds(1) - 1/c0 v_n v ds(2)) (demo/cpu_planar3d/forms.ufl:19-24)
is applied in its diagonal GLL form by wf_boundary_apply.

Not in the reference: leapfrog() integrates the same equation with the second-order central-difference scheme (one
stiffness apply per step, wf_leapfrog_step_bc), stable_time_step() gives a stable step for it.
sources= (points.Sources) adds point sources f = s(t) delta(x - x_s) to the right-hand side of the equation as the model
states it (u_tt - c0^2 Lap u = f; with a medium (1/(rho c^2)) p_tt - div((1/rho) grad p) = f): b[d] += s(t) phi_d(x_s) at
exactly the time argument at which each loop evaluates the plane source s1.  receivers= (points.Receivers) records u at
the start time and after every step of rk4 / rk4_fused / leapfrog (steps + 1 rows per call; trace_times).  With both
None the loops issue the launches they always did.

Ghost exchange: `updater` (a VectorUpdater) supplies scatter_fwd / scatter_rev
where the reference calls la::Vector::scatter_fwd / scatter_rev(add)
(LinearGLL.hpp:110,127,164,176,284-285); None on one rank.  The forward update
of v inside f1 (LinearGLL.hpp:167) is not needed here: the boundary term is
applied by the owner of each boundary dof with the fully assembled facet mass
(distributed.owned_boundary), so no ghost value of v is ever read."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import la
from ._lib import WAVE_RHS_FN, WAVE_STEP_FN, WF_WAVE_LEAPFROG, WF_WAVE_LEAPFROG4, WF_WAVE_RK4_FUSED, WaveDesc, WaveSource, _dp, _ip, check, lib
from .box import _int3
from .distributed import overlapped_apply
from .mesh_io import cfl_time_step  # noqa: F401  (demo/cpu_planar3d/main.cpp:48-66: one function for box and file meshes)
from .operators import CellForm, MassOperatorLumped, StiffnessOperator, _ptr, _stream


def facet_lumped_mass(V, tag_of_face, tag: int, cell_weight=None):
    """Collocated facet mass m_Gamma[i] = sum_facets w_q |J_facet| for the box
    faces carrying `tag` (tag_of_face maps local face 2*axis+side -> tag).
    cell_weight [ncells] (or None): every facet's contribution times the value of its cell.
    Host-side setup (wf_box_facet_mass: the loop of mesh_io.facet_lumped_mass on the implicit box numbering);
    returns (dof indices int32 ascending, masses float64)."""
    mesh = V.mesh
    if cell_weight is not None:
        cell_weight = np.ascontiguousarray(cell_weight, dtype=np.float64).reshape(-1)
        if cell_weight.size != mesh.ncells:
            raise ValueError(f"cell_weight has {cell_weight.size} entries, the mesh has {mesh.ncells} cells")
    x = np.ascontiguousarray(mesh.x, dtype=np.float64)
    face_tag = (ctypes.c_int * 6)(*(int(tag_of_face.get(f, 0)) for f in range(6)))
    nout = ctypes.c_int64(0)
    args = (V.degree, _int3(mesh.n), _dp(x), face_tag, int(tag), _dp(cell_weight), ctypes.byref(nout))
    check(lib().wf_box_facet_mass(*args, None, None))
    idx, m = np.empty(nout.value, dtype=np.int32), np.empty(nout.value)
    check(lib().wf_box_facet_mass(*args, _ip(idx), _dp(m)))
    return idx, m


class LinearGLLOpt:
    #: rk4_fused: the stage kernel leaves the next right-hand side's boundary term in b (wf_rk4_stage_bc).  False keeps
    #: the boundary term a launch of its own after each stage kernel, for comparison (tools/ab_rk4_boundary.py).
    fold_boundary = True
    _rec_T = None   # (receivers, their transpose as Sources) of misfit_gradient

    def __init__(self, V, degreeOfBasis: int, speedOfSound: float, sourceFrequency: float,
                 pressureAmplitude: float, boundary=None, updater=None, device=None, structured=None,
                 tags=None, tuning=None, medium=None, sources=None, receivers=None):
        if updater is not None and (sources is not None or receivers is not None):
            raise NotImplementedError("LinearGLLOpt: sources= / receivers= on a partitioned mesh (updater=) are not implemented; "
                                      "points.locate and the point kernels work on one rank's mesh")
        self.sources, self.receivers = sources, receivers
        if medium is not None:
            # (1/(rho c^2)) p_tt = div((1/rho) grad p), dp/dn = g on Gamma_1, dp/dn = -p_t / c on Gamma_2 (medium.py).
            # The facet masses of both boundary sets carry the admittance 1 / (rho c) of the facet's cell: derived from
            # tags they are weighted here; a caller's boundary= (a mesh read from a file) must carry it already --
            # mesh_io.boundary_sets(V, tags, cell_weight=medium.admittance).
            if updater is not None:
                raise NotImplementedError("LinearGLLOpt: medium= on a partitioned mesh (updater=) is not implemented; the "
                                          "operators themselves take per-local-cell coefficients on any partition")
            if medium.ncells != V.mesh.ncells:
                raise ValueError(f"medium has {medium.ncells} cells, the mesh has {V.mesh.ncells}")
        self.medium = medium
        self.V = V
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.k_ = degreeOfBasis
        self.c0_ = speedOfSound
        self.freq0_ = sourceFrequency
        self.p0_ = pressureAmplitude
        self.w0_ = 2.0 * math.pi * self.freq0_
        self.T_ = 1.0 / self.freq0_
        self.alpha_ = 4.0
        # the plane source as the library evaluates it (csrc/wave_source.h); c0 ** 2 is this front end's own c0^2
        c0 = 0.0 if medium is not None else float(self.c0_)
        self._wave = WaveSource(c0, c0 ** 2, self.p0_, self.w0_, self.freq0_, self.alpha_, self.T_, int(medium is not None))
        self.updater = updater
        self._structured = structured
        self._cell_forms = None   # (stiffness form, lumped-mass form), built on first use (cell_forms)
        self.size_local = V.index_map.size_local
        N = V.ndofs
        z = lambda: torch.zeros(N, dtype=torch.float64, device=self.device)
        self.u, self.v, self.u_n, self.v_n = z(), z(), z(), z()
        self.m, self.b = z(), z()
        # LinearGLL.hpp:102-110: m = M 1, then scatter_rev(add)
        ones = torch.ones(N, dtype=torch.float64, device=self.device)
        if medium is None:
            self.mass_op = MassOperatorLumped(V, self.k_, structured=structured)
        else:
            self.mass_op = MassOperatorLumped(V, self.k_, structured=structured, cell_coeff=medium.mass_coeff)
        self.mass_op(ones, self.m)
        if self.updater is not None:
            self.updater.scatter_rev(self.m)
            self.updater.scatter_fwd(self.m)   # keep ghost entries of m non-zero and consistent for b/m
        # LinearGLL.hpp:113-115: the boundary form
        if boundary is None:
            if tags is None:
                tags = {0: 1, 1: 2, 2: 2, 3: 2, 4: 2, 5: 2}
            if self.updater is not None:
                from .distributed import owned_boundary
                i1, m1 = owned_boundary(self.updater, V, tags, 1, self.device)
                i2, m2 = owned_boundary(self.updater, V, tags, 2, self.device)
            elif medium is not None:
                i1, m1 = facet_lumped_mass(V, tags, 1, medium.admittance)
                i2, m2 = facet_lumped_mass(V, tags, 2, medium.admittance)
            else:
                i1, m1 = facet_lumped_mass(V, tags, 1)
                i2, m2 = facet_lumped_mass(V, tags, 2)
        else:
            # boundary = ((idx1, m1), (idx2, m2)): rank-local sets (any mix of owned and ghost dofs, rank-local
            # facet masses).  On a partitioned mesh they go through the same accumulate-to-owner-and-filter
            # step as the tag-derived sets: the loop below applies the boundary term to owned dofs only and
            # never updates the ghosts of v (contract of owned_boundary_set).
            (i1, m1), (i2, m2) = boundary
            if self.updater is not None:
                from .distributed import owned_boundary_set
                i1, m1 = owned_boundary_set(self.updater, V, i1, m1, self.device)
                i2, m2 = owned_boundary_set(self.updater, V, i2, m2, self.device)
        td = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(self.device, dtype=dt)
        # the same sets as the fused passes read them.  Built here and not on a loop's first call: wf_boundary_create
        # allocates and copies synchronously, and the first loop queued behind other work would wait for that work
        self._bc = la.BoundaryPlan(N, i1, m1, i2, m2)
        self.idx1, self.mG1 = td(i1, torch.int32), td(m1, torch.float64)
        self.idx2, self.mG2 = td(i2, torch.int32), td(m2, torch.float64)
        # LinearGLL.hpp:120-127; tuning: the stiffness operator's make_tuning dict, e.g. {"geometry": "per_cell"}
        if medium is None:
            self.stiff_op = StiffnessOperator(V, self.k_, {"c0": self.c0_}, structured=structured, tuning=tuning)
        else:
            self.stiff_op = StiffnessOperator(V, self.k_, {"c0": 1.0}, structured=structured, tuning=tuning,
                                              cell_coeff=medium.stiff_coeff)
        # (the boundary term stays two scalars per stage: with a medium the facet masses carry the admittance 1 / (rho c),
        # s1(t) = window p0 w0 cos(w0 t) and s2 = -1: _boundary_scalars)
        # domain-decomposed run: interior cells overlap the forward ghost update
        self._split = False
        if self.updater is not None:
            self._split = self.stiff_op.set_ghost_faces(*[bool(v) for v in self.updater.part.owned_lo])
            if not self._split:   # arbitrary dofmap: split by the ghost positions the updater unpacks into
                self._split = self.stiff_op.set_ghost_dofs(self.updater.h_ghost_pos)
        self.stiff_op(self.u_n, self.b)
        if self.updater is not None:
            self.updater.scatter_rev(self.b)
        self.window_ = 0.0
        self.g_ = 0.0

    def init(self):
        self.u_n.zero_()
        self.v_n.zero_()

    @property
    def trace_times(self):
        """The time of every row of receivers.traces"""
        return [] if self.receivers is None else self.receivers.times

    # ---- the pieces every time loop shares: the plane source is the library's (csrc/wave_source.h) ----
    def _window(self, t: float) -> float:
        """The source's start-up ramp over alpha_ periods (LinearGLL.hpp:153-159)."""
        return lib().wf_wave_window(ctypes.byref(self._wave), t)

    def _g(self, t: float) -> float:
        """g(t) of LinearGLL.hpp:153-162 (no medium: with one g = s1 / c differs from cell to cell and only s1 exists)."""
        return lib().wf_wave_g(ctypes.byref(self._wave), t)

    @property
    def _s2(self) -> float:
        """Coefficient of the Gamma_2 term: -c0 (LinearGLL.hpp:175); -1 with a medium (admittance-weighted facet masses)."""
        return lib().wf_wave_s2(ctypes.byref(self._wave))

    def _boundary_scalars(self, t: float):
        """(s1, s2) of the boundary term b[idx1] += s1 mG1, b[idx2] += s2 mG2 v at time t: c0^2 g(t) and -c0
        (LinearGLL.hpp:153-162,175); with a medium window p0 w0 cos(w0 t) and -1 on admittance-weighted facet masses."""
        return self._s1(t), self._s2

    def _s1(self, t: float) -> float:
        """Coefficient of the Gamma_1 term at time t."""
        return lib().wf_wave_s1(ctypes.byref(self._wave), t)

    def _s1_fused(self, t: float) -> float:
        """_s1(t) as rk4_fused rounds it: the product taken from left to right (wave_source.h says why both stay)."""
        return lib().wf_wave_s1_left_to_right(ctypes.byref(self._wave), t)

    def _rhs(self, x, b):
        """b += K x with the ghost exchange of a partitioned mesh around it: forward halo of x, reverse halo of b."""
        if self._split:
            # interior cells beside the halo of x, the interface cells and the reverse halo of b
            overlapped_apply(self.stiff_op, self.updater, x, b)
            return
        if self.updater is not None:
            self.updater.scatter_fwd(x)
        self.stiff_op(x, b)
        if self.updater is not None:
            self.updater.scatter_rev(b)

    def f0(self, t, u, v, result):
        la.copy(v, result)                                   # LinearGLL.hpp:141-144

    def f1(self, t, u, v, result):
        # LinearGLL.hpp:151-192
        self.window_ = self._window(t)
        self.g_ = self._g(t) if self.medium is None else None
        s1, s2 = self._boundary_scalars(t)
        if self._split:
            # same operations as below, reordered so that the cells that read no ghost
            # value run while the halo of u is in flight (update_fwd_begin/_end,
            # VectorUpdater.hpp:106-143)
            la.fill(self.b, 0.0)
            self._rhs(u, self.b)
            la.boundary_apply(self.idx1, self.mG1, s1, self.idx2, self.mG2, s2, v, self.b)
            if self.sources is not None:
                self.sources.add(t, self.b)
            la.copy(u, self.u_n)
            la.copy(v, self.v_n)
            la.pointwise_div(self.b, self.m, result)
            return
        # the reference's order: the apply reads the copy u_n, the reverse halo of b follows the boundary term
        if self.updater is not None:
            self.updater.scatter_fwd(u)
        la.copy(u, self.u_n)
        la.copy(v, self.v_n)
        la.fill(self.b, 0.0)
        self.stiff_op(self.u_n, self.b)
        la.boundary_apply(self.idx1, self.mG1, s1, self.idx2, self.mG2, s2, self.v_n, self.b)
        if self.sources is not None:
            self.sources.add(t, self.b)
        if self.updater is not None:
            self.updater.scatter_rev(self.b)
        la.pointwise_div(self.b, self.m, result)

    def rk4(self, startTime: float, finalTime: float, timeStep: float, max_steps: int | None = None):
        # LinearGLL.hpp:198-287.  rk4, f0 and f1 are the line-by-line transcription of common/LinearGLL.hpp:141-287 and stay
        # readable as such, here and in wavehip_linear_gll.hpp; the loops the product runs are the library's (_run)
        t, tf, dt = startTime, finalTime, timeStep
        step = 0
        nl = self.size_local
        new = lambda: torch.zeros_like(self.u_n)
        u_, v_, un, vn, u0, v0, ku, kv = (new() for _ in range(8))
        la.copy(self.u_n, u_)
        la.copy(self.v_n, v_)
        la.copy(u_, ku)
        la.copy(v_, kv)
        a_runge = [0.0, 0.5, 0.5, 1.0]
        b_runge = [1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0]
        c_runge = [0.0, 0.5, 0.5, 1.0]
        rec = self.receivers
        if rec is not None:
            rec.record(u_, t)
        while t < tf:
            dt = min(dt, tf - t)
            la.copy(u_, u0)
            la.copy(v_, v0)
            for i in range(4):
                la.copy(u0, un)
                la.copy(v0, vn)
                la.axpy(un, dt * a_runge[i], ku, un, nl)
                la.axpy(vn, dt * a_runge[i], kv, vn, nl)
                tn = t + c_runge[i] * dt
                self.f0(tn, un, vn, ku)
                self.f1(tn, un, vn, kv)
                la.axpy(u_, dt * b_runge[i], ku, u_, nl)
                la.axpy(v_, dt * b_runge[i], kv, v_, nl)
            t += dt
            step += 1
            if rec is not None:
                rec.record(u_, t)
            if max_steps is not None and step >= max_steps:
                break
        la.copy(u_, self.u_n)
        la.copy(v_, self.v_n)
        if self.updater is not None:
            self.updater.scatter_fwd(self.u_n)
            self.updater.scatter_fwd(self.v_n)
        return t, step

    def rk4_fused(self, startTime: float, finalTime: float, timeStep: float, max_steps: int | None = None):
        """The same RK4 integration as rk4() (LinearGLL.hpp:198-287) with the vector
        algebra between two stiffness applies fused into one pass (wf_rk4_stage_bc) and
        the stage-0 copies removed by pointer rotation: per stage
        K (116 B/dof at P4) + 96 B/dof instead of K + 208 B/dof.  The diagonal boundary term
        of the NEXT right-hand side is left in b by the stage kernel (instead of zeros), so a
        stage is two launches: stiffness apply, fused vector algebra.  Same arithmetic
        expressions as the unfused loop (b receives the boundary term before the stiffness
        contributions instead of after them).  The loop itself is wf_wave_rk4_fused (csrc/wave_loops.cpp)."""
        return self._run(WF_WAVE_RK4_FUSED, startTime, finalTime, timeStep, max_steps)

    def leapfrog(self, startTime: float, finalTime: float, timeStep: float, max_steps: int | None = None):
        """Second-order central-difference (leapfrog, explicit Newmark beta = 0, gamma = 1/2) integration of
        m u'' + d u' - K u = s1(t) mG1, d = -s2 mG2 scattered to the dofs, from the state (u_n, v_n) to the state
        (u_n, v_n) like rk4(): ONE stiffness apply and one streaming pass (wf_leapfrog_step_bc, 48 B/dof) per step against
        the four applies of RK4.  The absorbing term is taken centred, d (u^{n+1} - u^{n-1}) / (2 dt): it is diagonal, so the
        implicit solve is a division, and the stability limit stays that of the undamped scheme, dt < 2 / sqrt(lambda_max)
        (stable_time_step) -- RK4 loses stability at dofs that carry several absorbing faces.

        Start-up: a^0 = (K u^0 + s1(t0) mG1 - d v^0) / m and u^{-1} = u^0 - dt v^0 + dt^2/2 a^0 (one apply).  Finish: one more
        apply and update into a scratch vector give v_n = (u^{n+1} - u^{n-1}) / (2 dt), the central velocity at the final
        time, without advancing u -- so a run split in two equals the continuous run up to rounding.

        The step is constant: steps are counted by `while t < finalTime` and the last step is NOT shortened to land on
        finalTime (a shortened step would break the two-level recurrence).  Returns (t, steps).  The loop itself is
        wf_wave_leapfrog (csrc/wave_loops.cpp)."""
        return self._run(WF_WAVE_LEAPFROG, startTime, finalTime, timeStep, max_steps)

    def leapfrog4(self, startTime: float, finalTime: float, timeStep: float, max_steps: int | None = None):
        """Fourth-order leapfrog (the modified-equation scheme, Lax-Wendroff on the two-level recurrence) of the same
        equation as leapfrog(), from (u_n, v_n) to (u_n, v_n):
            (u+ - 2u + u-) / dt^2 = A u + (dt^2/12) A^2 u,   A = M^-1 K,
        with the loads L and (dt^2/12)(A L + L'') beside it.  TWO stiffness applies and two streaming passes per step
        (wf_leapfrog4_predict 56 B/dof, wf_leapfrog4_correct 40 B/dof) against the four applies of RK4, at RK4's order.
        With x = dt^2 lambda_max the symbol x - x^2/12 stays in [0, 3] for 0 <= x <= 12: dt <= sqrt(12) / sqrt(lambda_max),
        sqrt(3) times leapfrog's limit (stable_time_step(scheme="leapfrog4")), with and without absorbing sets.

        The limit of the scheme: the centred absorbing term d u' stays SECOND order.  The result is fourth order on
        closed, reflecting and periodic domains and in the phase error that accumulates in the interior, second order in
        what the absorbing faces and their reflections contribute.  The order claim holds for Ricker wavelets and smooth
        loads; a sampled wavelet is piecewise linear and its second difference is not smooth.

        L' and L'' are central differences of the loads at t +- dt.  Start-up: a0, j0, q0 = the second to fourth time
        derivatives at t0 from three applies, u^{-1} = u0 - dt v0 + dt^2/2 a0 - dt^3/6 j0 + dt^4/24 q0.  Finish: one more
        full step into a scratch vector gives the central velocity vt and acceleration at; one more apply gives
        j = (K vt + L' - d at) / m and v_n = vt - dt^2/6 j (the plain central velocity is second order only); u is not
        advanced.  A run split in two equals the continuous run to TRUNCATION order, not to rounding: the start-up is a
        Taylor series, not the inverse of the finish.

        The step is constant and the last step is not shortened, as in leapfrog().  Returns (t, steps).  The loop itself is
        wf_wave_leapfrog4 (csrc/wave_loops.cpp)."""
        return self._run(WF_WAVE_LEAPFROG4, startTime, finalTime, timeStep, max_steps)

    def _guarded(self, errors, body):
        """body(*args) as a callback of the library (la.cg's trampoline): it runs under the stream the library hands over
        and lets no exception cross the C boundary -- the exception waits in `errors` for _run to raise it."""
        dev = self.device

        def call(stream, *args):
            try:
                # torch.cuda.ExternalStream(0) is NOT the null stream on ROCm (it wraps a bogus handle)
                st = torch.cuda.ExternalStream(stream, device=dev) if stream else torch.cuda.default_stream(dev)
                with torch.cuda.stream(st):
                    body(*args)
                return 0
            except Exception as e:   # noqa: BLE001
                errors.append(e)
                return -1
        return call

    def _run(self, scheme: int, t0: float, tf: float, dt: float, max_steps, keep=None, rhs=None, work=None, startup=None):
        """One call of wf_wave_rk4_fused / wf_wave_leapfrog / wf_wave_leapfrog4 on (u_n, v_n), by scheme: the
        descriptor, the work vectors and the trace rows are set up here, every launch is the library's.
        keep(n, t, u_prev, u, a0) (the two leapfrog loops; misfit_gradient) is called before step n = 0, 1, ... with the
        time and the two states the step reads; a0 is the vector holding the start-up acceleration, valid at n = 0 only
        (leapfrog), or startup[0] or None (leapfrog4).  It may copy them; the loop's own launches and their order do not
        depend on it.  startup (leapfrog4 alone): three vectors that receive a0, j0, q0 of the start-up.  For tests:
        rhs(x, b), a right-hand side b += K x in place of the model's, and work, the work vectors (wf_wave_work_vectors of
        them) in place of fresh ones.  Raises ValueError before any launch for what the library does not have: keep= with
        WF_WAVE_RK4_FUSED, startup= with another scheme than WF_WAVE_LEAPFROG4."""
        if keep is not None and scheme == WF_WAVE_RK4_FUSED:
            raise ValueError("LinearGLLOpt._run: keep= is the per-step callback of the leapfrog loops; wf_wave_rk4_fused has none")
        if startup is not None and scheme != WF_WAVE_LEAPFROG4:
            raise ValueError("LinearGLLOpt._run: startup= are the start-up derivatives of wf_wave_leapfrog4 alone")
        L, n, errors = lib(), self.u_n.numel(), []
        vec = lambda p: la._tensor_from_ptr(p, n, self.device) if p else None   # noqa: E731
        d = WaveDesc()
        d.n, d.d_m, d.d_b, d.bc = n, _ptr(self.m), _ptr(self.b), self._bc._h
        d.source, d.fold_boundary = self._wave, int(self.fold_boundary)
        if rhs is None and (self.updater is None or self.updater.transport == "native"):
            # the sequence of _rhs, in the library
            d.op, d.overlapped = self.stiff_op._h, int(self._split)
            if self.updater is not None and (self._split or self.updater.active):
                d.updater = self.updater._h
        else:   # the torch transport exchanges ghosts in Python: _rhs itself, as a callback
            body = self._rhs if rhs is None else rhs
            call = self._guarded(errors, lambda px, pb: body(vec(px), vec(pb)))
            d.rhs = WAVE_RHS_FN(lambda user, px, pb, stream: call(stream, px, pb))
        if self.sources is not None:
            d.sources = self.sources._s
        max_steps = -1 if max_steps is None else int(max_steps)
        rec = self.receivers
        if rec is not None:
            rows = L.wf_wave_step_count(scheme, t0, tf, dt, max_steps) + 1
            times = (ctypes.c_double * rows)()
            d.h_times, d.trace_rows = times, rows
            if len(rec):
                d.receivers, d.d_traces = rec._h, rec.reserve(rows, self.device)
        if work is None:
            work = [torch.empty_like(self.u_n) for _ in range(L.wf_wave_work_vectors(scheme))]
        d.d_work = (ctypes.c_void_p * len(work))(*[_ptr(x) for x in work])
        t_end, steps = ctypes.c_double(t0), ctypes.c_int64(0)
        args = (ctypes.byref(d), t0, tf, dt, max_steps, _ptr(self.u_n), _ptr(self.v_n))
        out = (ctypes.byref(t_end), ctypes.byref(steps), _stream(self.u_n))
        step_fn = WAVE_STEP_FN()
        if keep is not None:
            call_keep = self._guarded(errors, lambda k, t, pw, pu, pa: keep(k, t, vec(pw), vec(pu), vec(pa)))
            step_fn = WAVE_STEP_FN(lambda user, k, t, pw, pu, pa, stream: call_keep(stream, k, t, pw, pu, pa))
        if scheme == WF_WAVE_LEAPFROG4:
            kept = None if startup is None else (ctypes.c_void_p * 3)(*[_ptr(x) for x in startup])
            rc = L.wf_wave_leapfrog4(*args, step_fn, None, kept, *out)
        elif scheme == WF_WAVE_LEAPFROG:
            rc = L.wf_wave_leapfrog(*args, step_fn, None, *out)
        else:
            rc = L.wf_wave_rk4_fused(*args, *out)
        if errors:
            raise errors[0]
        check(rc)
        if rec is not None:
            rec.advance(list(times)[:steps.value + 1])
        if self.updater is not None:
            self.updater.scatter_fwd(self.u_n)
            self.updater.scatter_fwd(self.v_n)
        return t_end.value, int(steps.value)

    def misfit_gradient(self, t0: float, tf: float, dt: float, observed, checkpoint_every: int | None = None,
                        max_steps: int | None = None, scheme: str = "leapfrog"):
        """The L2 trace misfit of a leapfrog run and its gradient with respect to the cell coefficients of the model's two
        operators: returns (J, g_stiff, g_mass, info).

        The forward run is leapfrog(t0, tf, dt, max_steps) from the current (u_n, v_n): the same launches in the same
        order, recording u at `receivers` (rows n = 0 .. N, N the number of steps), and leaving u_n, v_n and
        receivers.traces as leapfrog would.  observed is [N + 1, R] (numpy or device) and

            J = 1/2 dt sum_n sum_r (traces[n, r] - observed[n, r])^2.

        g_stiff[c] = dJ/da^K_c and g_mass[c] = dJ/da^M_c are device vectors in the mesh's cell order; a^K, a^M are the cell
        coefficients of stiff_op and mass_op -- medium.stiff_coeff and medium.mass_coeff, or an implicit 1 per cell
        without a medium.  Held fixed: the facet masses mG1, mG2 (the admittance they carry included), s1(t), the sources,
        u^0 and v^0.  The chain rule to (c, rho) is the caller's, and exact only for cells without a tagged face.

        It is the gradient of the loop as it runs (the discrete adjoint), start-up included; the finishing step does not
        enter J.  With A+- = m +- h (h = hdt c2 on the boundary sets) step n is
            A+ u^{n+1} = dt^2 (K u^n + f^n) + 2 m u^n - A- u^{n-1},
        and the multipliers mu_N = mu_{N+1} = 0,
            A+ mu_{k-1} = dt^2 (K mu_k + R^T r^k / dt) + 2 m mu_k - A- mu_{k+1},        r^k = traces[k] - observed[k],
        march backwards through the same wf_leapfrog_step_bc (s1 = 0, the load by wf_sources_add_values on the transposed
        receivers): K is symmetric and m, h diagonal, so the adjoint absorbs with the same sign.  Then
            a^K_c g_stiff[c] = dt^2 (sum_n e^K_c(mu_n, u^n) + e^K_c(-1/2 (A-/m) mu_0, u^0)),
            a^M_c g_mass[c]  = e^M_c(1, q - p),   p = sum_n mu_n (u^{n+1} - 2 u^n + u^{n-1}),  q = dt^2/2 (A-/m) mu_0 a^0,
        with the forms of cell_forms() and p accumulated per step by wf_leapfrog_correlate (the lumped mass is diagonal).

        Memory: the forward run keeps the pair (u^{jS-1}, u^{jS}) every S = checkpoint_every steps (default
        ceil(sqrt(N))); the backward pass re-runs one segment at a time from its pair into S further vectors and marches
        mu back through it.  info: "N", "S", "vectors" (2 ceil(N/S) + min(S, N) + 5 vectors of ndofs doubles beyond the
        model's own: the pairs, the segment, mu twice, p, a^0, h), "bytes", "launches" (library calls that launch
        kernels), "t" and "steps" of the forward run.

        Re-running a segment repeats the launches of the forward run.  Where the stiffness apply is bitwise repeatable (the
        structured box's owner kernel, WF_FLAG_ORDERED) the replayed states, and so J and both gradients, are
        bit-identical for every S and from call to call; where the apply adds by atomics they agree to rounding only.

        scheme="leapfrog4": the same for the fourth-order loop, the forward run being leapfrog4(t0, tf, dt, max_steps) --
        _backward_leapfrog4 says what differs.

        Raises before the first launch: an unknown scheme, with updater=, without receivers, dt <= 0, observed of another
        shape, S < 1."""
        if scheme not in ("leapfrog", "leapfrog4"):
            raise ValueError(f"LinearGLLOpt.misfit_gradient: scheme must be 'leapfrog' or 'leapfrog4', got {scheme!r}")
        if self.updater is not None:
            raise NotImplementedError("LinearGLLOpt.misfit_gradient on a partitioned mesh (updater=) is not implemented")
        rec, src = self.receivers, self.sources
        if rec is None:
            raise ValueError("LinearGLLOpt.misfit_gradient needs receivers=")
        if not dt > 0.0:
            raise ValueError("LinearGLLOpt.misfit_gradient: the time step must be positive")
        N = lib().wf_wave_step_count(WF_WAVE_LEAPFROG, t0, tf, dt, -1 if max_steps is None else int(max_steps))   # the steps leapfrog will take
        R = len(rec)
        if tuple(observed.shape) != (N + 1, R):
            raise ValueError(f"LinearGLLOpt.misfit_gradient: observed is {tuple(observed.shape)}, the run records {(N + 1, R)}")
        S = max(1, math.isqrt(max(N - 1, 0)) + 1) if checkpoint_every is None else int(checkpoint_every)
        if S < 1:
            raise ValueError("LinearGLLOpt.misfit_gradient: checkpoint_every must be at least 1")
        if isinstance(observed, np.ndarray):
            observed = torch.from_numpy(np.array(observed, dtype=np.float64))   # a copy: the caller's array may be read-only
        observed = observed.to(self.device, dtype=torch.float64)
        fourth = scheme == "leapfrog4"
        ncp, Sb = -(-N // S), min(S, N)
        new = lambda: torch.empty_like(self.u_n)   # noqa: E731
        pairs, times = [], []
        kept = [new() for _ in range(4 if fourth else 1)]   # a0; with leapfrog4 also j0, q0 (the loop hands all three out) and v0

        def keep(n, tn, u_prev, u, scratch):
            times.append(tn)
            if n == 0 and not fourth:
                la.copy(scratch, kept[0])
            if n % S == 0:
                pair = (new(), new())
                la.copy(u_prev, pair[0])
                la.copy(u, pair[1])
                pairs.append(pair)

        row0 = rec._rows
        if fourth:
            la.copy(self.v_n, kept[3])
            t, steps = self._run(WF_WAVE_LEAPFROG4, t0, tf, dt, max_steps, keep, startup=kept[:3])
        else:
            t, steps = self._run(WF_WAVE_LEAPFROG, t0, tf, dt, max_steps, keep)
        assert steps == N and len(pairs) == ncp
        resid = rec.traces[row0:row0 + N + 1] - observed
        J = 0.5 * dt * float((resid * resid).sum().item())
        g_stiff = torch.zeros(self.V.mesh.ncells, dtype=torch.float64, device=self.device)
        ns = 0 if src is None else 1
        if fourth:
            vectors = 2 * ncp + 2 * Sb + 10
            launches = 36 + 6 * ns + N * (5 + 2 * ns) + 2 * ncp + (N * (4 + 2 * ns) + 5 * N + 3 * (N - 1) + 8 if N > 0 else 0)
        else:
            vectors = 2 * ncp + Sb + 5
            launches = (8 + ns + (N > 0)) + N * (3 + ns) + (3 + ns) + 2 * ncp + N * (2 + ns) + 5 * N + 2 * (N > 0)
        info = {"N": N, "S": S, "vectors": vectors, "t": t, "steps": steps, "launches": launches}
        info["bytes"] = info["vectors"] * self.u_n.numel() * 8
        if N == 0:
            return J, g_stiff, torch.zeros_like(g_stiff), info
        backward = self._backward_leapfrog4 if fourth else self._backward_leapfrog
        g_mass = backward(dt, N, S, pairs, times, resid, kept, g_stiff)
        if self.medium is not None:
            g_stiff.div_(torch.from_numpy(np.ascontiguousarray(self.medium.stiff_coeff)).to(self.device))
            g_mass.div_(torch.from_numpy(np.ascontiguousarray(self.medium.mass_coeff)).to(self.device))
        return J, g_stiff, g_mass, info

    def _receivers_transposed(self):
        """the receivers as sources (their transpose), built once per Receivers object"""
        if self._rec_T is None or self._rec_T[0] is not self.receivers:
            self._rec_T = (self.receivers, self.receivers.transpose())
        return self._rec_T[1]

    def _absorbing_masses(self):
        """c2: the facet masses mG2 scattered to the dofs, zero elsewhere"""
        c2 = torch.zeros_like(self.u_n)
        if self.idx2.numel():
            c2.index_add_(0, self.idx2.long(), self.mG2)
        return c2

    def _backward_leapfrog(self, dt, N, S, pairs, times, resid, kept, g_stiff):
        """The backward pass of misfit_gradient(scheme="leapfrog") behind the forward run (N > 0): accumulates
        a^K_c g_stiff[c] into g_stiff and returns a^M_c g_mass[c].  kept = [a0]."""
        src, b, m = self.sources, self.b, self.m
        ncp, Sb = len(pairs), min(S, N)
        kform, mform = self.cell_forms()
        RT = self._receivers_transposed()
        bc, s1, s2, rhs = self._bc, self._s1, self._s2, self._rhs
        mu, mu_next, p = torch.zeros_like(self.u_n), torch.zeros_like(self.u_n), torch.zeros_like(self.u_n)
        bufs = [torch.empty_like(self.u_n) for _ in range(Sb)]
        for j in reversed(range(ncp)):
            n0, n1 = j * S, min((j + 1) * S, N)
            st = [pairs[j][0], pairs[j][1]] + bufs[:n1 - n0]          # st[i] = u^{n0 - 1 + i}
            for i, n in enumerate(range(n0, n1)):                     # the forward steps of the segment again
                rhs(st[i + 1], b)
                if src is not None:
                    src.add(times[n], b)
                la.leapfrog_step(b, m, st[i + 1], st[i], st[i + 2], dt, bc=bc, s1=s1(times[n]), s2=s2)
            for n in reversed(range(n0, n1)):                         # mu_n from mu = mu_{n+1}, mu_next = mu_{n+2}
                i = n - n0
                rhs(mu, b)
                RT.add_values(resid[n + 1], b, scale=1.0 / dt)
                la.leapfrog_step(b, m, mu, mu_next, mu_next, dt, bc=bc, s1=0.0, s2=s2)
                mu, mu_next = mu_next, mu
                kform.eval(mu, st[i + 1], out=g_stiff, accumulate=True)
                la.leapfrog_correlate(mu, st[i + 2], st[i + 1], st[i], p)
            if j > 0:
                pairs[j] = None
        # start-up: u^{-1} = u^0 - dt v^0 + dt^2/2 a^0 depends on K and m; mu_next = (A-/m) mu_0
        u0, a0 = pairs[0][1], kept[0]
        h = self._absorbing_masses()
        h.mul_((-s2) * (0.5 * dt))
        torch.sub(m, h, out=mu_next)
        mu_next.div_(m).mul_(mu)
        kform.eval(mu_next, u0, out=g_stiff, alpha=-0.5, accumulate=True)
        mu_next.mul_(a0)
        p.mul_(-1.0).add_(mu_next, alpha=0.5 * dt * dt)               # q - p
        mu.fill_(1.0)
        g_mass = mform.eval(mu, p)
        g_stiff.mul_(dt * dt)
        return g_mass

    def _backward_leapfrog4(self, dt, N, S, pairs, times, resid, kept, g_stiff):
        """_backward_leapfrog for scheme="leapfrog4", kept = [a0, j0, q0, v0]: the discrete adjoint of the leapfrog4 loop
        (wf_leapfrog4_correlate in include/wavehip.h has the derivation in the loop's notation).  Step n is
            b1 = K u^n + F1^n,  u* = the leapfrog update,  w^n = c12 b1/m,  A+ u^{n+1} = A+ u* + dt^2 (K w^n + F2^n),
        that is A+ u^{n+1} = dt^2 K' u^n + 2 m u^n - A- u^{n-1} + loads with K' = K + c12 K m^-1 K symmetric, and
            mu_N = mu_{N+1} = 0,   A+ mu_{k-1} = dt^2 (K mu_k + K om_k + R^T r^k / dt) + 2 m mu_k - A- mu_{k+1},   om_k = c12 (K mu_k)/m
        is the forward step again: la.leapfrog4_predict on b = K mu_k with s1 = 0 leaves om_k in its w, the residual load
        goes onto b = K om_k AFTER it (before, it would flow into om), la.leapfrog4_correct with s1c = 0.  Per step n < N
            a^K_c g_stiff[c] += dt^2 (e^K_c(mu_n, u^n + w^n) + e^K_c(om_n, u^n)),
            p += mu_n (u^{n+1} - 2 u^n + u^{n-1}) + 12 om_n w^n          (la.leapfrog4_correlate, which also writes u^n + w^n),
        and the start-up, with nu = -A- mu_0 and d = -s2 c2:
            qh = (dt^4/24 nu)/m,  jh = (-dt^3/6 nu - d qh)/m,  ah = (dt^2/2 nu + K qh - d jh)/m,
            a^K_c g_stiff[c] += e^K_c(qh, a0) + e^K_c(jh, v0) + e^K_c(ah, u0),   p += qh q0 + jh j0 + ah a0,
        and a^M_c g_mass[c] = e^M_c(1, -p).  The backward pass takes two applies a step: om_n comes out of the predictor half
        of the iteration that forms mu_{n-1}, so each iteration is predictor half, the step's terms, (the replay of the
        segment before, where n opens one,) corrector half.

        Memory: the pairs (u^{jS-1}, u^{jS}) as for leapfrog, and u^n AND w^n of one segment.  info["vectors"] =
        2 ceil(N/S) + 2 min(S, N) + 10: the pairs, the segment, and mu twice, om, p, u + w, a0, j0, q0, v0, h.
        info["launches"] = 36 + 6 s + N (5 + 2 s) + 2 ceil(N/S), the forward run with its copies, and with N > 0 a further
        N (4 + 2 s) + 5 N + 3 (N - 1) + 8: the replays, the predictor halves with the step's terms, the corrector halves,
        and mu_{N-1} with the start-up terms (s = 1 with sources)."""
        src, b, m = self.sources, self.b, self.m
        ncp, Sb = len(pairs), min(S, N)
        a0, j0, q0, v0 = kept
        new = lambda: torch.empty_like(self.u_n)   # noqa: E731
        kform, mform = self.cell_forms()
        RT = self._receivers_transposed()
        bc, s1, s2, rhs = self._bc, self._s1, self._s2, self._rhs
        dt2 = dt * dt
        mu, mu_next, om = torch.zeros_like(self.u_n), torch.zeros_like(self.u_n), new()
        p, z = torch.zeros_like(self.u_n), new()
        ubuf, wbuf = [new() for _ in range(Sb)], [new() for _ in range(Sb)]

        def states(j):
            """st[i] = u^{jS - 1 + i} of segment j"""
            return [pairs[j][0], pairs[j][1]] + ubuf[:min((j + 1) * S, N) - j * S]

        def replay(j):
            """the forward steps of segment j again, from its pair: the launches of wf_wave_leapfrog4's step"""
            st = states(j)
            for i, n in enumerate(range(j * S, min((j + 1) * S, N))):
                tn = times[n]
                rhs(st[i + 1], b)
                if src is not None:
                    src.add(tn, b)
                la.leapfrog4_predict(b, m, st[i + 1], st[i], st[i + 2], wbuf[i], dt, bc=bc, s1=s1(tn), s2=s2)
                rhs(wbuf[i], b)
                if src is not None:
                    src.add_stencil((tn - dt, tn, tn + dt), (1.0 / 12.0, -2.0 * (1.0 / 12.0), 1.0 / 12.0), b)
                s1c = ((s1(tn + dt) - 2.0 * s1(tn)) + s1(tn - dt)) / 12.0
                la.leapfrog4_correct(b, m, st[i + 2], st[i + 2], dt, bc=bc, s1c=s1c, s2=s2)

        # mu_{N-1} from mu_N = mu_{N+1} = 0: the predictor half of zeros is zeros, b holds the residual load alone
        RT.add_values(resid[N], b, scale=1.0 / dt)
        la.leapfrog4_correct(b, m, mu_next, mu, dt, bc=bc, s1c=0.0, s2=s2)
        replay(ncp - 1)
        st = states(ncp - 1)
        for n in reversed(range(N)):                                  # mu = mu_n, mu_next = mu_{n+1}
            j, i = divmod(n, S)
            rhs(mu, b)
            la.leapfrog4_predict(b, m, mu, mu_next, mu_next, om, dt, bc=bc, s1=0.0, s2=s2)     # om = om_n, mu_next = mu*
            la.leapfrog4_correlate(mu, om, st[i + 2], st[i + 1], st[i], wbuf[i], p, z)
            kform.eval(mu, z, out=g_stiff, accumulate=True)
            kform.eval(om, st[i + 1], out=g_stiff, accumulate=True)
            if i == 0 and j > 0:
                pairs[j] = None
                replay(j - 1)
                st = states(j - 1)
            if n > 0:
                rhs(om, b)
                RT.add_values(resid[n], b, scale=1.0 / dt)
                la.leapfrog4_correct(b, m, mu_next, mu_next, dt, bc=bc, s1c=0.0, s2=s2)
                mu, mu_next = mu_next, mu
        g_stiff.mul_(dt2)
        # start-up: u^{-1} = u0 - dt v0 + dt^2/2 a0 - dt^3/6 j0 + dt^4/24 q0 depends on K and m through a0, j0, q0.
        # mu holds mu_0; nu goes into mu_next, qh into om, jh into mu, ah into mu_next; z holds d
        u0 = pairs[0][1]
        h = self._absorbing_masses()
        torch.mul(h, -s2, out=z)                                      # d = -s2 c2
        h.mul_((-s2) * (0.5 * dt))
        torch.sub(h, m, out=mu_next)
        mu_next.mul_(mu)                                              # nu = -A- mu_0
        torch.mul(mu_next, (dt2 * dt2) / 24.0, out=om)
        om.div_(m)                                                    # qh
        torch.mul(mu_next, -(dt2 * dt) / 6.0, out=mu)
        mu.addcmul_(z, om, value=-1.0).div_(m)                        # jh
        rhs(om, b)                                                    # b = K qh (the corrector left it zero)
        mu_next.mul_(0.5 * dt2).add_(b).addcmul_(z, mu, value=-1.0).div_(m)   # ah
        la.fill(b, 0.0)
        kform.eval(om, a0, out=g_stiff, accumulate=True)
        kform.eval(mu, v0, out=g_stiff, accumulate=True)
        kform.eval(mu_next, u0, out=g_stiff, accumulate=True)
        p.addcmul_(om, q0).addcmul_(mu, j0).addcmul_(mu_next, a0)
        p.mul_(-1.0)
        z.fill_(1.0)
        return mform.eval(z, p)

    def max_eigenvalue(self, iters: int = 100):
        """Largest eigenvalue of -M^{-1} K (lumped mass, the model's stiffness operator) by `iters` power iterations; the
        value returned is the Rayleigh quotient -x^T K x / x^T M x of the last iterate.  It approaches lambda_max from
        BELOW (a Rayleigh quotient never exceeds it): on small P2 and P4 boxes it was 0.9992 and 0.9995 of the converged
        value after 100 iterations and 0.996 after 50, so keep a safety factor in the step derived from it.  One rank."""
        if self.updater is not None:
            raise NotImplementedError("LinearGLLOpt.max_eigenvalue on a partitioned mesh (updater=) is not implemented")
        if iters < 1:
            raise ValueError("max_eigenvalue needs at least one iteration")
        n = self.m.numel()
        x = torch.from_numpy(np.random.default_rng(0).uniform(-1.0, 1.0, n)).to(self.device)
        y, mx = torch.zeros_like(x), torch.zeros_like(x)
        lam = 0.0
        for _ in range(iters):
            la.fill(y, 0.0)
            self.stiff_op(x, y)                                  # y = K x
            la.fill(mx, 0.0)
            la.pointwise_mult_add(self.m, x, mx)                 # mx = M x
            lam = -la.inner_product(x, y) / la.inner_product(x, mx)
            la.pointwise_div(y, self.m, mx)                      # next iterate M^{-1} K x, normalised
            nrm = math.sqrt(la.inner_product(mx, mx))
            if not nrm > 0.0:
                break
            la.scale(1.0 / nrm, mx)
            x, mx = mx, x
        return lam

    def stable_time_step(self, safety: float = 0.9, iters: int = 100, scheme: str = "leapfrog"):
        """safety * 2 / sqrt(lambda_max(-M^{-1} K)): a stable step of leapfrog() (its limit is 2 / sqrt(lambda_max), with or
        without the absorbing term).  max_eigenvalue approaches lambda_max from below, so the limit is overestimated by
        up to ~0.04 % after 100 iterations; safety covers it.  scheme="leapfrog4": sqrt(3) times that, a stable step of
        leapfrog4() (limit sqrt(12) / sqrt(lambda_max)).  One rank."""
        if scheme not in ("leapfrog", "leapfrog4"):
            raise ValueError(f"stable_time_step: scheme must be 'leapfrog' or 'leapfrog4', got {scheme!r}")
        dt = safety * 2.0 / math.sqrt(self.max_eigenvalue(iters))
        return dt * math.sqrt(3.0) if scheme == "leapfrog4" else dt

    def cell_forms(self):
        """(stiffness form, lumped-mass form) of the model's operators: operators.CellForm with the model's c0, or with
        the medium's stiff_coeff / mass_coeff as cell_coeff.  Built on first use and kept.  One rank."""
        if self.updater is not None:
            raise NotImplementedError("LinearGLLOpt.cell_forms on a partitioned mesh (updater=) is not implemented")
        if self._cell_forms is None:
            if self.medium is None:
                self._cell_forms = (CellForm(self.V, self.k_, "stiffness", {"c0": self.c0_}, structured=self._structured),
                                    CellForm(self.V, self.k_, "mass_lumped", structured=self._structured))
            else:
                self._cell_forms = (CellForm(self.V, self.k_, "stiffness", {"c0": 1.0}, structured=self._structured,
                                             cell_coeff=self.medium.stiff_coeff),
                                    CellForm(self.V, self.k_, "mass_lumped", structured=self._structured,
                                             cell_coeff=self.medium.mass_coeff))
        return self._cell_forms

    def cell_energy(self, out=None):
        """The discrete energy per cell, 1/2 e^M_c(v_n, v_n) - 1/2 e^K_c(u_n, u_n) (K carries its minus sign, so both
        terms are non-negative); its sum is 1/2 v^T (m .* v) - 1/2 u^T K u.  Returns out [ncells].  One rank."""
        if self.updater is not None:
            raise NotImplementedError("LinearGLLOpt.cell_energy on a partitioned mesh (updater=) is not implemented")
        kform, mform = self.cell_forms()
        out = mform.eval(self.v_n, self.v_n, out=out, alpha=0.5)
        return kform.eval(self.u_n, self.u_n, out=out, alpha=-0.5, accumulate=True)
