"""Point sources and point receivers: locate physical points in the mesh, record the degree-P field there and load
point forces, all on the device (wf_points_*, wf_sources_* of include/wavehip.h; csrc/point_locate.cpp, csrc/points.hip).

Not in the reference: its only source is the plane term on the faces tagged 1 and its only output a whole dof vector.

A source is the right-hand side f = s(t) delta(x - x_s) of the equation as the model states it,

    u_tt - c0^2 Lap u = f                              without a medium,
    (1/(rho c^2)) p_tt - div((1/rho) grad p) = f       with one;

in both cases its load on the right-hand side vector is b[d] += s(t) phi_d(x_s).

Reference coordinates are those of tabulate_gll: [0, 1]^3.

Out of scope: partitioned meshes, tetrahedra, moving sources, moment-tensor or derivative sources, recording v inside
the time loops (Receivers.sample works on any vector), trace file formats."""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib
from ._lib import Handle, _dp, _ip, check, lib
from .operators import _check_vec, _ptr, _stream

#: tolerance of locate(): a cell accepts a point whose reference coordinates lie in [-TOL/2, 1 + TOL/2]
TOL = 1e-10


def locate(V, xyz, tol: float = TOL):
    """(cell [npoints] int32, ref [npoints][3]) of the physical points xyz in the mesh of V (wf_points_locate), from
    V.mesh.x and V.mesh.geom_dofmap -- box meshes and meshes read from files alike.  cell is -1 for a point in no cell;
    a point shared by several cells goes to the lowest cell index."""
    x = np.ascontiguousarray(V.mesh.x, dtype=np.float64)
    cells = np.ascontiguousarray(V.mesh.geom_dofmap, dtype=np.int32)
    p = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
    cell = np.empty(p.shape[0], dtype=np.int32)
    ref = np.empty((p.shape[0], 3))
    check(lib().wf_points_locate(x.shape[0], _dp(x), cells.shape[0], _ip(cells), p.shape[0], _dp(p), float(tol), _ip(cell), _dp(ref)))
    return cell, ref


def weights(degree: int, ref):
    """[npoints][3][degree + 1]: the 1-D Lagrange basis on the GLL nodes at each reference coordinate
    (wf_points_weights; barycentric form, exact 0/1 rows at the nodes)."""
    r = np.ascontiguousarray(np.asarray(ref, dtype=np.float64).reshape(-1, 3))
    w = np.empty((r.shape[0], 3, max(int(degree), 0) + 1))
    check(lib().wf_points_weights(int(degree), r.shape[0], _dp(r), _dp(w)))
    return w


def merge_sources(degree: int, dofs, w):
    """(dof, off, src, weight): the CSR over the unique dofs of point sources with dofmap rows dofs [nsrc][nd] and
    weights w [nsrc][3][degree + 1], as Sources builds it (wf_sources_merge)."""
    d = np.ascontiguousarray(dofs, dtype=np.int32)
    ww = np.ascontiguousarray(w, dtype=np.float64)
    nu, ne = ctypes.c_int32(0), ctypes.c_int32(0)
    args = (int(degree), d.shape[0], _ip(d), _dp(ww), ctypes.byref(nu), ctypes.byref(ne))
    check(lib().wf_sources_merge(*args, None, None, None, None))
    dof, off = np.empty(nu.value, dtype=np.int32), np.empty(nu.value + 1, dtype=np.int32)
    src, wt = np.empty(ne.value, dtype=np.int32), np.empty(ne.value)
    check(lib().wf_sources_merge(*args, _ip(dof), _ip(off), _ip(src), _dp(wt)))
    return dof, off, src, wt


def ricker(frequency: float, delay: float, amplitude: float = 1.0) -> dict:
    """s(t) = amplitude (1 - 2a) e^{-a}, a = (pi frequency (t - delay))^2"""
    if not (frequency > 0.0 and math.isfinite(frequency) and math.isfinite(delay) and math.isfinite(amplitude)):
        raise ValueError("ricker: frequency must be positive, delay and amplitude finite")
    return {"kind": "ricker", "frequency": float(frequency), "delay": float(delay), "amplitude": float(amplitude)}


def sampled(values, t_start: float, dt: float) -> dict:
    """s(t) = linear interpolation of `values` on t_start + k dt, zero outside the table (the half-stage times of RK4
    fall between the nodes of a table sampled at the time step)."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    if v.size < 2:
        raise ValueError(f"sampled: a table needs at least 2 samples, got {v.size}")
    if not (dt > 0.0 and math.isfinite(dt) and math.isfinite(t_start)):
        raise ValueError(f"sampled: dt must be positive and t_start finite, got dt = {dt}")
    if not np.isfinite(v).all():
        raise ValueError("sampled: a sample is not finite")
    return {"kind": "sampled", "values": v, "t_start": float(t_start), "dt": float(dt), "amplitude": 1.0}


def wavelet_value(wavelet: dict, t: float) -> float:
    """s(t) on the host in float64: the expressions wf_sources_add evaluates on the device."""
    if wavelet["kind"] == "ricker":
        a = (math.pi * wavelet["frequency"] * (t - wavelet["delay"])) ** 2
        return 0.0 if not a < 800.0 else wavelet["amplitude"] * ((1.0 - 2.0 * a) * math.exp(-a))
    v = wavelet["values"]
    u = (t - wavelet["t_start"]) / wavelet["dt"]
    if not (0.0 <= u <= v.size - 1):
        return 0.0
    k = min(int(u), v.size - 2)
    th = u - k
    return wavelet["amplitude"] * ((1.0 - th) * float(v[k]) + th * float(v[k + 1]))


class _Points(Handle):
    """wf_points: located points with their dofmap rows and weights on the device.  located = (cell [n], ref [n][3]), a
    public keyword of Receivers and Sources: the points are given by their cell and reference coordinates in [0, 1]^3 and
    xyz is not looked at -- for a caller who has located them already, or wants a point exactly on a node."""
    _destroy = "wf_points_destroy"

    def __init__(self, V, xyz, what: str, located=None):
        self.V = V
        if located is not None:      # (cell, ref) known to the caller: xyz is not looked at
            self.xyz = None
            self.cell = np.ascontiguousarray(located[0], dtype=np.int32).reshape(-1)
            self.ref = np.ascontiguousarray(np.asarray(located[1], dtype=np.float64).reshape(-1, 3))
            if self.ref.shape[0] != self.cell.size or (self.cell.size and (self.cell.min() < 0 or self.cell.max() >= V.mesh.ncells)):
                raise ValueError(f"{what}: located = (cell [n], ref [n][3]) with cells of the mesh")
        else:
            self.xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
            self.cell, self.ref = locate(V, self.xyz)
        missing = np.nonzero(self.cell < 0)[0]
        if missing.size:
            i = int(missing[0])
            raise ValueError(f"{what}: point {i} at {tuple(self.xyz[i])} lies in no cell of the mesh")
        self.w = weights(V.degree, self.ref)
        self.dofs = np.ascontiguousarray(np.asarray(V.dofmap)[self.cell], dtype=np.int32).reshape(self.cell.size, -1)
        self._h = ctypes.c_void_p()
        check(lib().wf_points_create(int(V.degree), int(V.ndofs), self.cell.size, _ip(self.dofs) if self.cell.size else None,
                                     _dp(self.w) if self.cell.size else None, ctypes.byref(self._h)))

    def __len__(self):
        return int(self.cell.size)


class Receivers(_Points):
    """Receivers(V, xyz): sample(x) evaluates the field x at the points (wf_points_sample: one wavefront per point, a
    fixed summation order, so a trace does not depend on which other receivers exist); record(x) appends a row to a
    device buffer that doubles when full; traces is the [rows, R] view of what was recorded, times the matching list of
    times.  Raises ValueError naming the first point that lies in no cell."""

    def __init__(self, V, xyz, device=None, capacity: int = 64, located=None):
        """located = (cell, ref): points given by cell and reference coordinates instead of xyz"""
        super().__init__(V, xyz, "Receivers", located)
        self.device = device
        self._buf = None
        self._rows = 0
        self._capacity = max(int(capacity), 1)
        self.times: list = []

    def sample(self, x, out=None):
        """out[r] = x at receiver r; out (optional) is a contiguous float64 device vector of len(self) entries, which may
        be a slice of a larger buffer."""
        import torch
        _check_vec(x, self.V.ndofs, "Receivers.sample x")
        if out is None:
            out = torch.empty(len(self), dtype=torch.float64, device=x.device)
        _check_vec(out, len(self), "Receivers.sample out")
        check(lib().wf_points_sample(self._h, _ptr(x), _ptr(out), _stream(x)))
        return out

    def reserve(self, rows: int, device) -> int:
        """Room for `rows` more rows -- the buffer doubles until they fit -- and the device pointer of the next row, for a
        writer that fills them itself (the time loops of the library); advance() then counts them."""
        import torch
        R = len(self)
        if self._buf is None:
            self._buf = torch.zeros(self._capacity * R, dtype=torch.float64, device=device)
        size = self._buf.numel()
        while size < (self._rows + rows) * R:
            size *= 2
        if size > self._buf.numel():
            grown = torch.zeros(size, dtype=torch.float64, device=device)
            grown[:self._buf.numel()].copy_(self._buf)
            self._buf = grown
        return self._buf.data_ptr() + self._rows * R * 8

    def advance(self, times):
        """Count the rows a writer filled behind reserve(), one per entry of times."""
        self._rows += len(times)
        self.times.extend(times)

    def record(self, x, t: float | None = None):
        """Append x at the receivers as one row of traces (time t, if given, to times)."""
        R = len(self)
        self.reserve(1, x.device)
        if R:
            self.sample(x, self._buf[self._rows * R:(self._rows + 1) * R])
        self.advance([t])

    @property
    def traces(self):
        """[rows, R] view of the recorded rows (device tensor; empty before the first record)"""
        import torch
        if self._buf is None:
            return torch.zeros((self._rows, len(self)), dtype=torch.float64, device=self.device)
        R = len(self)
        return self._buf[:self._rows * R].view(self._rows, R)

    def reset(self):
        self._rows = 0
        self.times = []

    def transpose(self):
        """Sources on the same located points (the same cells and reference coordinates, so the same weights) with
        zero-amplitude wavelets: its add_values(r, b) is b += R^T r where sample(x) is R x."""
        return Sources(self.V, None, [ricker(1.0, 0.0, 0.0)] * len(self), located=(self.cell, self.ref))


class Sources(_Points):
    """Sources(V, xyz, wavelets): point sources f = s_i(t) delta(x - x_i), wavelets a list of ricker(...) / sampled(...)
    descriptors, one per point.  add(t, b) does b[d] += sum_i s_i(t) phi_d(x_i) in one launch (wf_sources_add: the
    sources merged into a CSR over their unique dofs, one writer per dof, no atomics, the wavelets evaluated on the
    device).  Raises ValueError naming the first point that lies in no cell."""

    def __init__(self, V, xyz, wavelets, located=None):
        wavelets = list(wavelets)
        n = np.asarray(xyz, dtype=np.float64).reshape(-1, 3).shape[0] if located is None else np.asarray(located[0]).size
        if len(wavelets) != n:
            raise ValueError(f"Sources: {n} points but {len(wavelets)} wavelets")
        super().__init__(V, xyz, "Sources", located)
        self.wavelets = wavelets
        arr = (_lib.Wavelet * max(n, 1))()
        keep = []
        for i, wl in enumerate(wavelets):
            arr[i].amplitude = wl["amplitude"]
            if wl["kind"] == "ricker":
                arr[i].kind, arr[i].frequency, arr[i].delay = _lib.WF_WAVELET_RICKER, wl["frequency"], wl["delay"]
            elif wl["kind"] == "sampled":
                v = np.ascontiguousarray(wl["values"], dtype=np.float64)
                keep.append(v)
                arr[i].kind, arr[i].nsamples, arr[i].h_samples = _lib.WF_WAVELET_SAMPLED, v.size, _dp(v)
                arr[i].t_start, arr[i].dt = wl["t_start"], wl["dt"]
            else:
                raise ValueError(f"Sources: unknown wavelet kind {wl['kind']!r}")
        point_of = np.arange(n, dtype=np.int32)
        self._s = ctypes.c_void_p()
        check(lib().wf_sources_create(self._h, n, _ip(point_of) if n else None, arr, ctypes.byref(self._s)))
        _Points.close(self)      # the sources hold their own CSR: the plan's device rows and weights are not needed again

    @property
    def num_unique_dofs(self) -> int:
        nu = ctypes.c_int(0)
        check(lib().wf_sources_info(self._s, None, ctypes.byref(nu), None))
        return nu.value

    def add(self, t: float, b):
        """b[d] += sum_i s_i(t) phi_d(x_i)"""
        _check_vec(b, self.V.ndofs, "Sources.add b")
        check(lib().wf_sources_add(self._s, float(t), _ptr(b), _stream(b)))

    def add_stencil(self, times, weights, b):
        """b[d] += sum_i S_i phi_d(x_i), S_i = ((a_0 s_i(t_0)) + a_1 s_i(t_1)) + a_2 s_i(t_2) over the one to three (times,
        weights) given: a difference quotient of the load in one launch (wf_sources_add_stencil)."""
        t = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        a = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if t.size != a.size:
            raise ValueError(f"Sources.add_stencil: {t.size} times but {a.size} weights")
        _check_vec(b, self.V.ndofs, "Sources.add_stencil b")
        check(lib().wf_sources_add_stencil(self._s, int(t.size), _dp(t), _dp(a), _ptr(b), _stream(b)))

    def add_values(self, values, b, scale: float = 1.0):
        """b[d] += scale * sum_i values[i] phi_d(x_i): the wavelets are not looked at, values (a contiguous float64 device
        vector of len(self) entries, which may be a row of a larger buffer) takes their place (wf_sources_add_values)."""
        _check_vec(values, len(self), "Sources.add_values values")
        _check_vec(b, self.V.ndofs, "Sources.add_values b")
        check(lib().wf_sources_add_values(self._s, _ptr(values), float(scale), _ptr(b), _stream(b)))

    def close(self):
        if getattr(self, "_s", None) is not None and self._s.value:
            lib().wf_sources_destroy(self._s)
        self._s = None
        super().close()
