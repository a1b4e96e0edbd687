"""Host-side mirror of the reference's operator classes on top of libwavehip.

Same names, argument meaning and error behaviour as the reference:
  StiffnessOperator(V, bdegree, params)      common/operators.hpp:137-201
  MassOperatorLumped(V, bdegree)             common/operators.hpp:44-109 (MassOperatorCPU)
  SpectralMassOperator(V, bdegree)           common/cuda/spectral_mass.hpp:24-100
  MassOperator(V, element, quad_type, qd)    common/cuda/mass.hpp:18-107
  gather / scatter / transform1              common/cuda/scatter.hpp, transform.hpp
`op(x, y)` and `op.apply(x, y)` both compute y += A x on device vectors
(torch.float64 CUDA tensors, or anything with data_ptr()).  Failures raise
WavehipError (the reference throws std::runtime_error)."""
from __future__ import annotations

import ctypes
from ctypes import c_double, c_int32, c_void_p

import numpy as np

from . import _lib
from ._lib import OpDesc, OpInfo, _dp, _ip, check, lib
from .box import FunctionSpace


def _ptr(t) -> int:
    if isinstance(t, int):
        return t
    return int(t.data_ptr())


def _stream(t=None) -> int:
    """The HIP stream the call is ordered on: torch's current stream for the
    tensor's device (plumbing only)."""
    try:
        import torch
        if t is not None and hasattr(t, "is_cuda") and t.is_cuda:
            return int(torch.cuda.current_stream(t.device).cuda_stream)
    except ImportError:
        pass
    return 0


def _check_vec(t, n: int, name: str):
    if hasattr(t, "dtype"):
        import torch
        if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
            raise _lib.WavehipError(f"{name}: expected a contiguous float64 device vector")
        if t.numel() < n:
            raise _lib.WavehipError(f"{name}: vector has {t.numel()} entries, operator needs {n}")


def _cell_coeff(cell_coeff, ncells: int):
    """A cell coefficient argument as the contiguous float64 array [ncells] the C ABI takes, or None."""
    if cell_coeff is None:
        return None
    a = np.ascontiguousarray(cell_coeff, dtype=np.float64).reshape(-1)
    if a.size != ncells:
        raise _lib.WavehipError(f"cell_coeff has {a.size} entries, the mesh has {ncells} cells")
    return a


# ---------------------------------------------------------------------------
# setup functions (a1, a2)
# ---------------------------------------------------------------------------
def tabulate_gll(p: int):
    """1-D GLL points, weights and collocation derivative matrix D[q][a]."""
    n = p + 1
    pts, wts, D = np.zeros(n), np.zeros(n), np.zeros((n, n))
    check(lib().wf_tabulate_gll(p, _dp(pts), _dp(wts), _dp(D)))
    return pts, wts, D


def tabulate_dense(p: int):
    """tabulate_basis_and_permutation (common/operators.hpp:13-32): returns
    (perm, table[4][nq][nd]); perm is the identity in this engine's ordering."""
    nd = (p + 1) ** 3
    table = np.zeros((4, nd, nd))
    check(lib().wf_tabulate_dense(p, _dp(table)))
    return np.arange(nd, dtype=np.int32), table


_QUAD = {"gll": _lib.WF_QUAD_GLL, "gauss_jacobi": _lib.WF_QUAD_GAUSS_JACOBI}
_VARIANT = {"gll_warped": _lib.WF_VARIANT_GLL_WARPED, "gll": _lib.WF_VARIANT_GLL_WARPED, "equispaced": _lib.WF_VARIANT_EQUISPACED}


def quadrature_1d(quad: str, degree: int):
    """basix::quadrature::make_quadrature(quad, interval, degree) on [0,1]: (points, weights).
    "gauss_jacobi" has (degree+2)//2 points, "gll" (degree+4)//2 (precompute.hpp:183-184,
    operators.hpp:19)."""
    n = ctypes.c_int(0)
    pts, wts = np.zeros(_lib.WF_MAX_QUAD_POINTS), np.zeros(_lib.WF_MAX_QUAD_POINTS)
    check(lib().wf_quadrature_1d(_QUAD[quad], int(degree), ctypes.byref(n), _dp(pts), _dp(wts)))
    return pts[: n.value].copy(), wts[: n.value].copy()


def tabulate_1d(p: int, points, derivative: int = 0, variant: str = "gll_warped"):
    """tabulate_1d(p, q, derivative) of common/precompute.hpp:179-189 at given points:
    table[q][a] = l_a(x_q) or l_a'(x_q) for the degree-p Lagrange basis of `variant`."""
    pts = np.ascontiguousarray(points, dtype=np.float64)
    out = np.zeros((pts.size, p + 1))
    check(lib().wf_tabulate_1d(p, _VARIANT[variant], pts.size, _dp(pts), int(derivative), _dp(out)))
    return out


def compute_geometry_rule(mesh, points1, weights1, use_fabs: bool = False, clamp: bool = False, want_G: bool = False):
    """compute_jacobian / _determinant / compute_geometrical_factor of
    common/precompute.hpp:49-176 at the tensor rule points1^3: (G or None, detJ*w)."""
    pts = np.ascontiguousarray(points1, dtype=np.float64)
    wts = np.ascontiguousarray(weights1, dtype=np.float64)
    nq = pts.size ** 3
    x = np.ascontiguousarray(mesh.x, dtype=np.float64)
    gd = np.ascontiguousarray(mesh.geom_dofmap, dtype=np.int32)
    G = np.zeros((mesh.ncells, nq, 3, 3)) if want_G else None
    detJ = np.zeros((mesh.ncells, nq))
    check(lib().wf_geometry_hex_rule(mesh.ncells, x.shape[0], _dp(x), _ip(gd), pts.size, _dp(pts), _dp(wts),
                                     int(use_fabs), int(clamp), _dp(G), _dp(detJ)))
    return G, detJ


def hex_cell_geometry(mesh, p: int, use_fabs: bool = True, clamp: bool = True):
    """The per-cell geometry of affine hexahedra and the test that allows it (wf_geometry_hex_cell, host only, no
    device needed): (Gc[ncells][6] = G00 G01 G02 G11 G12 G22 of J^-1 J^-T |det J|, first_bad, reason).  first_bad is -1
    when every cell qualifies, else the first cell that does not (Gc is complete only below it); reason 0 ok, 1 not
    affine (edge vectors along a reference axis not bitwise equal), 2 det J zero or not finite, 3 the reference's
    -1/0/1 clamp would take effect at the degree-p rule.  This is the rule behind tuning={"geometry": "per_cell"}."""
    x = np.ascontiguousarray(mesh.x, dtype=np.float64)
    gd = np.ascontiguousarray(mesh.geom_dofmap, dtype=np.int32)
    ncells = gd.size // 8
    Gc = np.zeros((ncells, 6))
    bad, reason = ctypes.c_int64(-1), ctypes.c_int(0)
    check(lib().wf_geometry_hex_cell(p, ncells, x.shape[0], _dp(x), _ip(gd), int(use_fabs), int(clamp), _dp(Gc),
                                     ctypes.byref(bad), ctypes.byref(reason)))
    return Gc, int(bad.value), int(reason.value)


def precompute_geometric_data(mesh, p: int, use_fabs: bool = True, clamp: bool = True, want_G: bool = True):
    """precompute_geometric_data (common/precomputation.hpp:18-110) on the device;
    returns host arrays (G[ncells][nq][3][3], detJ[ncells][nq])."""
    nq = (p + 1) ** 3
    x = np.ascontiguousarray(mesh.x, dtype=np.float64)
    gd = np.ascontiguousarray(mesh.geom_dofmap, dtype=np.int32)
    G = np.zeros((mesh.ncells, nq, 3, 3)) if want_G else None
    detJ = np.zeros((mesh.ncells, nq))
    check(lib().wf_geometry_hex(p, mesh.ncells, x.shape[0], _dp(x), _ip(gd), int(use_fabs), int(clamp),
                                _dp(G), _dp(detJ)))
    return G, detJ


# ---------------------------------------------------------------------------
# operator handles
# ---------------------------------------------------------------------------
def make_tuning(tuning) -> "_lib.Tuning | None":
    """wf_tuning from a dict (kernel=, variant=, lz=, lz0=, block=(bx, by, bz), keep_cell_order=, orient=, geometry=,
    metric=, update=) or None.  `kernel` is a WF_KERNEL_FORCE_* value or one of "batch", "box_block", "mass_any",
    "elementwise", "march", "mass_march" (dense mass with a rectangular 1-D table: the marching kernel on request; raises
    WavehipError for a (degree, rule points) pair that is not compiled and on any other operator); `geometry` a wf_geometry_mode value or one of "auto", "per_point", "per_cell"; `metric` a
    wf_metric_mode value or one of "auto", "full", "axes"; `update` a wf_update_mode value or one of "auto", "atomic",
    "owner".  {"update": "owner"} gives the owner-computes separable box stiffness kernel (per-cell geometry, no atomics,
    bitwise reproducible) on a rectilinear box at degrees 1 to 7 and raises WavehipError on any other mesh; `variant`
    then indexes its three cross-sections.  "auto" picks it at degree 4 only; at degrees 5 to 7 "auto" keeps the k-split
    kernel with per-point geometry.  On an operator of any dofmap (structured=False, a mesh read from a file)
    {"geometry": "per_cell"} stores one G_c per cell at degrees 1 to 4 when every cell is affine (hex_cell_geometry) and
    raises WavehipError otherwise; "metric" then chooses between the full and the separable form as on a box, and
    "auto" / "per_point" keep the per-point kernel."""
    if tuning is None:
        return None
    if isinstance(tuning, _lib.Tuning):
        return tuning
    names = {"auto": 0, "batch": _lib.WF_KERNEL_FORCE_BATCH, "box_block": _lib.WF_KERNEL_FORCE_BOX_BLOCK,
             "mass_any": _lib.WF_KERNEL_FORCE_MASS_ANY, "elementwise": _lib.WF_KERNEL_FORCE_ELEMENTWISE,
             "march": _lib.WF_KERNEL_FORCE_MARCH, "mass_march": _lib.WF_KERNEL_FORCE_MASS_MARCH}
    t = _lib.Tuning()
    k = tuning.get("kernel", 0)
    t.kernel = names[k] if isinstance(k, str) else int(k)
    t.variant = int(tuning.get("variant", -1)) + 1       # C ABI: compiled cross-section + 1, 0 = default
    t.lz = int(tuning.get("lz", 0))
    t.lz0 = int(tuning.get("lz0", 0))
    t.bx, t.by, t.bz = (int(v) for v in tuning.get("block", (0, 0, 0)))
    t.keep_cell_order = int(bool(tuning.get("keep_cell_order", False)))
    t.orient = int(tuning.get("orient", 0))
    g = tuning.get("geometry", 0)
    t.geometry = GEOMETRY_MODES[g] if isinstance(g, str) else int(g)
    m = tuning.get("metric", 0)
    t.metric = METRIC_MODES[m] if isinstance(m, str) else int(m)
    u = tuning.get("update", 0)
    t.update = UPDATE_MODES[u] if isinstance(u, str) else int(u)
    return t


GEOMETRY_MODES = {"auto": 0, "per_point": 1, "per_cell": 2}
METRIC_MODES = {"auto": 0, "full": 1, "axes": 2}
UPDATE_MODES = {"auto": 0, "atomic": 1, "owner": 2}
KERNEL_NAMES = {0: "none", 1: "march_box", 2: "march_idx", 3: "batch_unique", 4: "box_block", 5: "diagonal",
                6: "mass_dense_any", 7: "dense_simplex", 8: "elementwise", 9: "cells_ordered",
                10: "dense_simplex_mass"}


GEOMETRY_NAMES = {1: "per_point", 2: "per_cell"}    # wf_op_info_t.geometry, wf_cell_form_info_t.geometry


def _structured_default(V, *arrays) -> bool:
    """structured=None: the box entry point when V says its dofmap is the lexicographic box numbering and the caller
    hands over no array (G, detJ, perm) that only the dofmap entry point takes."""
    return bool(getattr(V, "structured", False)) and all(a is None for a in arrays)


def _hex_desc(V: FunctionSpace, kind: int, degree: int, perm=None, c0: float = 0.0, flags: int = 0, G=None, detJ=None,
              cell_coeff=None, tuning=None):
    """The wf_op_desc of the dofmap entry points (wf_op_create, wf_cell_form_create) and the arrays it points into,
    which the caller holds until the call has returned: (desc, keep).  The geometry is G [ncells][nq][3][3] or detJ
    where given, else V's mesh."""
    d = OpDesc()
    d.kind, d.degree, d.ncells, d.ndofs = kind, degree, V.mesh.ncells, V.ndofs
    d.c0, d.flags = c0, flags
    dm = np.ascontiguousarray(V.dofmap, dtype=np.int32)
    if dm.shape != (V.mesh.ncells, (degree + 1) ** 3):
        raise _lib.WavehipError("dofmap shape does not match ncells x (degree+1)^3")
    pm = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
    d.h_dofmap, d.h_perm = _ip(dm), _ip(pm)
    keep = [dm, pm]
    if G is not None:
        Gc = np.ascontiguousarray(G, dtype=np.float64)
        if Gc.size != V.mesh.ncells * (degree + 1) ** 3 * 9:
            raise _lib.WavehipError("G must be [ncells][nq][3][3]")
        keep.append(Gc)
        d.h_G = _dp(Gc)
    elif detJ is not None:
        keep.append(np.ascontiguousarray(detJ, dtype=np.float64))
        d.h_detJ = _dp(keep[-1])
    else:
        x = np.ascontiguousarray(V.mesh.x, dtype=np.float64)
        gd = np.ascontiguousarray(V.mesh.geom_dofmap, dtype=np.int32)
        keep += [x, gd]
        d.nverts, d.h_xverts, d.h_geom_dofmap = x.shape[0], _dp(x), _ip(gd)
    a, t = _cell_coeff(cell_coeff, d.ncells), make_tuning(tuning)
    keep += [a, t]
    d.h_cell_coeff = _dp(a)
    if t is not None:
        d.tuning = ctypes.pointer(t)
    return d, keep


def _create_on_box(create, handle, kind: int, p: int, mesh, c0: float, flags: int, tuning, cell_coeff):
    """wf_op_create_box_coeff or wf_cell_form_create_box (one argument list) on the box `mesh`"""
    nx, ny, nz = mesh.n
    x = np.ascontiguousarray(mesh.x, dtype=np.float64)
    a = _cell_coeff(cell_coeff, nx * ny * nz)
    t = make_tuning(tuning)
    check(create(kind, p, nx, ny, nz, _dp(x), float(c0), _dp(a), flags, ctypes.byref(t) if t is not None else None,
                 ctypes.byref(handle)))


class _Operator(_lib.Handle):
    _destroy = "wf_op_destroy"

    def __init__(self):
        self._h = c_void_p()

    def _create(self, desc: OpDesc, keep):
        check(lib().wf_op_create(ctypes.byref(desc), ctypes.byref(self._h)))   # keep: the arrays desc points into
        self._info()

    def _create_box(self, kind: int, p: int, mesh, c0: float, flags: int, tuning=None, cell_coeff=None):
        _create_on_box(lib().wf_op_create_box_coeff, self._h, kind, p, mesh, c0, flags, tuning, cell_coeff)
        self._info()

    @property
    def cell_coeff(self) -> bool:
        """Whether the operator was created with a cell coefficient array (wf_op_info_t.cell_coeff)."""
        return bool(self.info.cell_coeff)

    @property
    def kernel(self) -> str:
        """Name of the kernel wf_op_apply launches (wf_op_info_t.kernel)."""
        return KERNEL_NAMES.get(self.info.kernel, "?")

    @property
    def geometry(self) -> str:
        """How the stiffness geometry is stored (wf_op_info_t.geometry): "per_point", "per_cell" or "none"."""
        return GEOMETRY_NAMES.get(self.info.geometry, "none")

    @property
    def metric(self) -> str:
        """Form of the per-cell kernel, box or dofmap (wf_op_info_t.metric): "full", "axes" or "none" (no per-cell
        geometry)."""
        return {1: "full", 2: "axes"}.get(self.info.metric, "none")

    @property
    def update(self) -> str:
        """How the separable box kernel adds into y (wf_op_info_t.update): "atomic", "owner" or "none" (another
        kernel); "ordered" for an operator created with WF_FLAG_ORDERED (order-fixed accumulation: every y entry summed
        by one thread in the order of the caller's dofmap, bitwise reproducible on any mesh)."""
        return {1: "atomic", 2: "owner", 3: "ordered"}.get(self.info.update, "none")

    def _info(self):
        info = OpInfo()
        check(lib().wf_op_info(self._h, ctypes.byref(info)))
        self.info = info

    # introspection as common/cuda/mass.hpp:68-71
    def num_quads(self): return self.info.num_quads
    def num_cells(self): return self.info.num_cells
    def num_dofs(self): return self.info.num_dofs_cell
    def flops(self): return self.info.flops
    def alg_bytes(self): return self.info.alg_bytes

    def apply(self, x, y, stream: int | None = None):
        """y += A x (accumulate; the caller zeroes y, LinearGLL.hpp:173)."""
        _check_vec(x, self.info.ndofs, "x")
        _check_vec(y, self.info.ndofs, "y")
        s = _stream(x) if stream is None else stream
        check(lib().wf_op_apply(self._h, _ptr(x), _ptr(y), s))

    __call__ = apply

    def set_ghost_faces(self, gx: bool, gy: bool, gz: bool) -> bool:
        """Declare which lower lattice planes are ghost planes (domain
        decomposition, box operators).  Returns False when this operator cannot be
        split this way: the caller then uses set_ghost_dofs or the unsplit sequence."""
        rc = lib().wf_op_set_ghost_faces(self._h, int(gx), int(gy), int(gz))
        if rc == -2:
            return False
        check(rc)
        self._info()
        return True

    def set_ghost_dofs(self, ghost_positions) -> bool:
        """Interior / interface split from the ghost positions of the local array (the
        list the VectorUpdater unpacks into): works for every marching operator, box or
        arbitrary dofmap.  Returns False for operators that run a batch kernel."""
        g = np.ascontiguousarray(ghost_positions, dtype=np.int32)
        rc = lib().wf_op_set_ghost_dofs(self._h, _ip(g) if g.size else None, int(g.size))
        if rc == -2:
            return False
        check(rc)
        self._info()
        return True

    def replan_runs(self, resident: int = 0):
        """Plan the whole apply of a box owner operator again, for `resident` workgroups (0: the occupancy query, as at
        creation).  The interior / interface parts keep their z segments."""
        check(lib().wf_op_replan_runs(self._h, int(resident)))
        self._info()

    def set_runs(self, runs):
        """Install a run table of the caller's, [runs][3] = (column, z0, z1) per workgroup in launch order; it must
        cover every layer of every column exactly once.  An empty table drops the operator's."""
        r = np.ascontiguousarray(runs, dtype=np.int32).reshape(-1, 3)
        check(lib().wf_op_set_runs(self._h, _ip(r) if r.size else None, r.shape[0]))
        self._info()

    def runs(self):
        """The run table of the whole apply, [runs][3] = (column, z0, z1) per workgroup; empty without one."""
        n = c_int32(0)
        check(lib().wf_op_get_runs(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros((n.value, 3), dtype=np.int32)
        if n.value:
            check(lib().wf_op_get_runs(self._h, _ip(out), n.value, ctypes.byref(n)))
        return out

    def part_fraction(self, part: int) -> float:
        """Share of the operator's work items in `part` (after set_ghost_faces)."""
        tot = self.info.items_interior + self.info.items_interface
        if tot == 0:
            return 1.0
        return (self.info.items_interior if part == 1 else self.info.items_interface) / tot

    def apply_part(self, x, y, part: int, stream: int | None = None):
        """y += A_part x, part in (WF_PART_INTERIOR, WF_PART_INTERFACE):
        interior cells read no ghost value of x."""
        _check_vec(x, self.info.ndofs, "x")
        _check_vec(y, self.info.ndofs, "y")
        s = _stream(x) if stream is None else stream
        check(lib().wf_op_apply_part(self._h, _ptr(x), _ptr(y), part, s))


class StiffnessOperator(_Operator):
    """StiffnessOperator(V, bdegree, params) -- common/operators.hpp:137-201.

    params["c0"] is honoured (the reference hard-codes 1500, operators.hpp:114,
    which is the only value its caller passes).  G=None computes the geometry on
    the device from V.mesh (precomputation.hpp:69-107); a host array in the
    reference layout [ncells][nq][3][3] is used as given.
    structured=None picks the implicit-dofmap box kernel when V says its dofmap
    is the lexicographic box numbering; structured=False forces the generic
    (arbitrary dofmap, atomic scatter) kernel.  There tuning={"geometry": "per_cell"}
    asks for one G_c per cell (degrees 1 to 4, every cell affine, G=None): the
    marching kernel on lattice columns then streams 48 B per cell instead of 48 B
    per point; op.geometry, op.metric report what was built.

    cell_coeff (every operator class of this module): one value a_c per cell in the mesh's cell order, or
    None.  The operator is then sum_c a_c P_c^T A_c P_c with A_c the cell matrix without it (here with -c0^2
    and the clamp applied first); the values are folded into the stored geometry at creation, so the apply
    runs the same kernel at the same cost.  None is the operator as it always was."""

    def __init__(self, V: FunctionSpace, bdegree: int, params: dict | None = None, G=None, perm=None,
                 structured: bool | None = None, flags: int = 0, tuning=None, cell_coeff=None):
        super().__init__()
        c0 = 1500.0 if not params else float(params.get("c0", 1500.0))
        self.c0 = c0
        if _structured_default(V, G, perm) if structured is None else structured:
            if bdegree != V.degree:
                raise _lib.WavehipError("structured operator: bdegree must equal the space's degree")
            self._create_box(_lib.WF_OP_STIFFNESS, bdegree, V.mesh, c0, flags, tuning, cell_coeff)
            return
        self._create(*_hex_desc(V, _lib.WF_OP_STIFFNESS, bdegree, perm, c0, flags, G=G, cell_coeff=cell_coeff, tuning=tuning))


class MassOperatorLumped(_Operator):
    """MassOperatorCPU(V, bdegree) -- common/operators.hpp:44-109: the GLL-lumped
    mass y += M x.  detJ = |det J| w (fabs), as precompute_geometric_data."""

    def __init__(self, V: FunctionSpace, bdegree: int, detJ=None, perm=None, structured: bool | None = None,
                 flags: int = 0, tuning=None, cell_coeff=None):
        super().__init__()
        if _structured_default(V, detJ, perm) if structured is None else structured:
            self._create_box(_lib.WF_OP_MASS_LUMPED, bdegree, V.mesh, 0.0, flags, tuning if flags & _lib.WF_FLAG_ORDERED else None,
                             cell_coeff)
            return
        self._create(*_hex_desc(V, _lib.WF_OP_MASS_LUMPED, bdegree, perm, 0.0, flags, detJ=detJ, cell_coeff=cell_coeff,
                                tuning=tuning))


class CellForm(_lib.Handle):
    """Cell form of an operator: e_c(lambda, u) = (P_c lambda)^T A_c (P_c u), one number per cell (wf_cell_form,
    include/wavehip.h).  A_c is the cell matrix the operator of the same arguments stores: for kind="stiffness" with
    -c0^2, the clamp and cell_coeff, for kind="mass_lumped" cell_coeff det J w.  Without cell_coeff e_c is the
    derivative of lambda^T A u with respect to the cell's coefficient; with lambda = u the cell's share of the energy.

    The constructor arguments and the box / dofmap choice (`structured`) are those of StiffnessOperator and
    MassOperatorLumped.  tuning may hold "geometry" only ("auto": one G_c per cell where every cell is affine, else G
    per point; "per_point"; "per_cell": raises WavehipError naming the first cell that does not qualify).  The result
    is in the mesh's cell order, bitwise reproducible, and independent of where a cell sits in that order."""

    KINDS = {"stiffness": _lib.WF_OP_STIFFNESS, "mass_lumped": _lib.WF_OP_MASS_LUMPED, "mass_dense": _lib.WF_OP_MASS_DENSE}
    _destroy = "wf_cell_form_destroy"

    def __init__(self, V: FunctionSpace, degree: int, kind: str = "stiffness", params: dict | None = None, G=None,
                 detJ=None, perm=None, structured: bool | None = None, cell_coeff=None, tuning=None, flags: int = 0):
        self._h = c_void_p()
        if kind not in self.KINDS:
            raise _lib.WavehipError(f"CellForm: kind must be one of {sorted(self.KINDS)}")
        k = self.KINDS[kind]
        self.kind = kind
        self.c0 = 1500.0 if not params else float(params.get("c0", 1500.0))
        if _structured_default(V, G, detJ, perm) if structured is None else structured:
            if degree != V.degree:
                raise _lib.WavehipError("structured cell form: degree must equal the space's degree")
            _create_on_box(lib().wf_cell_form_create_box, self._h, k, degree, V.mesh, self.c0, flags, tuning, cell_coeff)
        else:
            stiffness = k == _lib.WF_OP_STIFFNESS
            d, keep = _hex_desc(V, k, degree, perm, self.c0, flags, G=G if stiffness else None,
                                detJ=None if stiffness else detJ, cell_coeff=cell_coeff, tuning=tuning)
            check(lib().wf_cell_form_create(ctypes.byref(d), ctypes.byref(self._h)))
        info = _lib.CellFormInfo()
        check(lib().wf_cell_form_info(self._h, ctypes.byref(info)))
        self.info = info

    @property
    def geometry(self) -> str:
        """How the stiffness form stores its geometry: "per_point", "per_cell", or "none" (lumped mass)."""
        return GEOMETRY_NAMES.get(self.info.geometry, "none")

    def eval(self, lam, u, out=None, alpha: float = 1.0, accumulate: bool = False, stream: int | None = None):
        """out[c] = (out[c] if accumulate else 0) + alpha e_c(lam, u); returns out (a new device vector when None).
        lam may be u.  Any number of evaluations may be in flight on different streams."""
        _check_vec(lam, self.info.ndofs, "lam")
        _check_vec(u, self.info.ndofs, "u")
        if out is None:
            if accumulate:
                raise _lib.WavehipError("CellForm.eval: accumulate needs out")
            import torch
            out = torch.empty(self.info.num_cells, dtype=torch.float64, device=u.device)
        _check_vec(out, self.info.num_cells, "out")
        s = _stream(u) if stream is None else stream
        check(lib().wf_cell_form_eval(self._h, _ptr(lam), _ptr(u), float(alpha), int(bool(accumulate)), _ptr(out), s))
        return out

    __call__ = eval


class SpectralMassOperator(MassOperatorLumped):
    """SpectralMassOperator(V, bdegree) -- common/cuda/spectral_mass.hpp:24-100.
    Same lumped mass; detJ = det(J) w WITHOUT fabs (spectral_mass.hpp:58-64 via
    precompute.hpp:102-116).  Degrees outside 2..7 are rejected like the
    reference's qdegree map (spectral_mass.hpp:42-48)."""

    def __init__(self, V: FunctionSpace, bdegree: int, structured: bool | None = None, cell_coeff=None):
        if bdegree < 2 or bdegree > 7:
            raise _lib.WavehipError("SpectralMassOperator: degree must be 2..7")
        super().__init__(V, bdegree, structured=structured, flags=_lib.WF_FLAG_NO_FABS, cell_coeff=cell_coeff)


class MassOperator(_Operator):
    """MassOperator(V, element, quad_type, qd) -- common/cuda/mass.hpp:18-107:
    y += Phi^T diag(detJ w) Phi x with a tensor-product rule.

    Either the reference's arguments -- the element as (degree, variant in
    {"gll_warped", "equispaced"}), quad in {"gll", "gauss_jacobi"} and the quadrature
    degree qdegree (mass.hpp:20-21; demo/gpu_operator/main.cpp:66-68,96-99 uses
    equispaced + gauss_jacobi of degree 2P) -- from which the 1-D table
    (tabulate_1d) and det J * w at the rule's points (on the device) are built; or
    explicit tables: `phi1` [nq1][P+1] and `detJ` [ncells][nq1^3] (mass.hpp:35-39)."""

    def __init__(self, V: FunctionSpace, degree: int, phi1: np.ndarray | None = None, detJ: np.ndarray | None = None,
                 perm=None, variant: str = "gll_warped", quad: str = "gll", qdegree: int | None = None, tuning=None,
                 flags: int = 0, cell_coeff=None):
        super().__init__()
        if phi1 is None:
            if qdegree is None:
                qdegree = degree + 1 if degree > 1 else degree      # gpu_operator_monolithic/main.cpp:95
            pts, wts = quadrature_1d(quad, qdegree)
            phi1 = tabulate_1d(degree, pts, 0, variant)
            self.points1, self.weights1 = pts, wts
        p1 = np.ascontiguousarray(phi1, dtype=np.float64)
        if p1.ndim != 2 or p1.shape[1] != degree + 1:
            raise _lib.WavehipError("phi1 must be [nq1][degree+1]")
        if detJ is not None and np.size(detJ) != V.mesh.ncells * p1.shape[0] ** 3:
            raise _lib.WavehipError("detJ must be [ncells][nq1^3]")
        if detJ is None and not hasattr(self, "points1"):
            raise _lib.WavehipError("MassOperator: explicit phi1 needs detJ")
        d, keep = _hex_desc(V, _lib.WF_OP_MASS_DENSE, degree, perm, 0.0, flags, detJ=detJ, cell_coeff=cell_coeff, tuning=tuning)
        keep.append(p1)
        d.nq1 = p1.shape[0]
        d.h_phi1 = _dp(p1)
        if detJ is None:
            d.flags |= _lib.WF_FLAG_NO_FABS   # mass.hpp:35-39: det J * w keeps its sign (compute_jacobian_determinant)
            qp, qw = np.ascontiguousarray(self.points1), np.ascontiguousarray(self.weights1)
            keep += [qp, qw]
            d.h_qpts1, d.h_qwts1 = _dp(qp), _dp(qw)
        self._create(d, keep)


# ---------------------------------------------------------------------------
# free kernels (common/cuda/scatter.hpp:7-14, transform.hpp:7-8)
# ---------------------------------------------------------------------------
def gather(N: int, indices, inp, out, block_size: int = 512, stream: int | None = None):
    """out[i] = in[indices[i]] (block_size accepted for signature parity, unused)."""
    check(lib().wf_gather(N, _ptr(indices), _ptr(inp), _ptr(out), _stream(inp) if stream is None else stream))


def scatter(N: int, indices, inp, out, block_size: int = 512, stream: int | None = None):
    """out[indices[i]] += in[i] (hardware fp64 atomics)."""
    check(lib().wf_scatter_add(N, _ptr(indices), _ptr(inp), _ptr(out), _stream(inp) if stream is None else stream))


def scatter_set(N: int, indices, inp, out, stream: int | None = None):
    check(lib().wf_scatter_set(N, _ptr(indices), _ptr(inp), _ptr(out), _stream(inp) if stream is None else stream))


def ordered_slots(dofmap, ndofs: int):
    """The plan of the order-fixed accumulation (wf_ordered_slots, host only): a stable counting sort of the flattened
    dofmap [ncells][nd].  Returns (row_off[ndofs + 1], slot[ncells][nd]): the contributions of dof d occupy the slots
    row_off[d] .. row_off[d+1]-1 in the order in which the dofmap lists d."""
    dm = np.ascontiguousarray(dofmap, dtype=np.int32)
    if dm.ndim != 2:
        raise _lib.WavehipError("ordered_slots: dofmap must be [ncells][nd]")
    row_off = np.zeros(int(ndofs) + 1, dtype=np.int32)
    slot = np.zeros(dm.shape, dtype=np.int32)
    check(lib().wf_ordered_slots(dm.shape[0], dm.shape[1], int(ndofs), _ip(dm), _ip(row_off), _ip(slot)))
    return row_off, slot


def box_run_plan(ncols: int, nz: int, resident: int, nxcd: int = 8, prologue: float = 1.5, lz: int = 0):
    """The z segmentation of a box marching operator of ncols columns and nz layers on `resident` workgroups
    (wf_box_run_plan, host only).  Returns (runs, cost, uniform_cost, uniform_lz): runs[r] = (column, z0, z1) of workgroup
    r, an empty [0][3] array when the uniform plan of uniform_lz layers per segment stays; costs in layers."""
    runs = np.zeros((int(ncols) * int(nz), 3), dtype=np.int32)
    n, ulz = c_int32(0), c_int32(0)
    cost, ucost = c_double(0.0), c_double(0.0)
    check(lib().wf_box_run_plan(int(ncols), int(nz), int(resident), int(nxcd), float(prologue), int(lz), _ip(runs),
                                runs.shape[0], ctypes.byref(n), ctypes.byref(cost), ctypes.byref(ucost), ctypes.byref(ulz)))
    return runs[:n.value].copy(), cost.value, ucost.value, ulz.value


def segment_sum_add(n: int, row_off, vals, y, stream: int | None = None):
    """y[d] += vals[row_off[d]] + vals[row_off[d]+1] + ... (summed front to back by one thread, no atomics) for d < n
    (wf_segment_sum_add): pass 2 of the order-fixed accumulation.  row_off: int32 device tensor [n + 1]."""
    check(lib().wf_segment_sum_add(int(n), _ptr(row_off), _ptr(vals), _ptr(y), _stream(y) if stream is None else stream))


def transform1(N: int, inp, detJ, out, block_size: int = 512, stream: int | None = None):
    """out[i] = in[i] * detJ[i]."""
    check(lib().wf_transform1(N, _ptr(inp), _ptr(detJ), _ptr(out), _stream(inp) if stream is None else stream))


def tsmm(ncells: int, inp, phi, out, layout: int = 0, stream: int | None = None):
    """out[cell][n] = sum_k in[cell][k] phi[k][n] (wf_tsmm; demo/gpu_tsmm, demo/gpu_operator DGEMMs).
    phi: device tensor [K][N] row-major."""
    K, N = int(phi.shape[0]), int(phi.shape[1])
    check(lib().wf_tsmm(layout, ncells, K, N, _ptr(inp), _ptr(phi), _ptr(out), _stream(inp) if stream is None else stream))
