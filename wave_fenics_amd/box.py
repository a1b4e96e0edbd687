"""Host-side box mesh and function-space descriptors.

Stand-ins for the DOLFINx objects the reference passes to its operators
(mesh::create_box + fem::create_functionspace, demo/gpu_operator/main.cpp:60-72):
plain numpy arrays with this engine's lexicographic numbering
(vertex (a,b,c) -> a + (nx+1)(b + (ny+1)c); dof (I,J,K) -> I + NX(J + NY K);
element-local tensor index l = i + n(j + n k))."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import _dp, _ip, check, lib


@dataclass
class IndexMap:
    """dolfinx::common::IndexMap as far as the operators use it: owned dofs
    first, ghosts after (operators use size_local + num_ghosts as array length)."""
    size_local: int
    num_ghosts: int = 0
    size_global: int | None = None

    def __post_init__(self):
        if self.size_global is None:
            self.size_global = self.size_local


@dataclass
class BoxMesh:
    n: tuple                   # cells per direction
    x: np.ndarray              # vertices [nv][3] float64
    geom_dofmap: np.ndarray    # [ncells][8] int32
    lo: tuple = (0.0, 0.0, 0.0)
    hi: tuple = (1.0, 1.0, 1.0)

    @property
    def ncells(self) -> int:
        return int(self.geom_dofmap.shape[0])


@dataclass
class FunctionSpace:
    mesh: BoxMesh
    degree: int
    dofmap: np.ndarray         # [ncells][nd] int32, tensor order
    index_map: IndexMap
    lattice: tuple             # (NX, NY, NZ)
    structured: bool = True    # dofmap is the implicit lexicographic box numbering

    @property
    def ndofs(self) -> int:
        return self.index_map.size_local + self.index_map.num_ghosts


def lattice_numbering(V: "FunctionSpace") -> np.ndarray:
    """Setup-time renumbering option (wf_lattice_numbering): new index of every dof of V in a numbering that follows
    the lattice columns the marching kernels walk.  For spaces whose own numbering scatters a cell's dofs over
    memory (a uniformly random numbering costs 2.8x in the stiffness apply)."""
    dm = np.ascontiguousarray(V.dofmap, dtype=np.int32)
    out = np.empty(V.ndofs, dtype=np.int32)
    check(lib().wf_lattice_numbering(V.degree, dm.shape[0], V.ndofs, _ip(dm), _ip(out)))
    return out


def renumber(V: "FunctionSpace", new_of_old: np.ndarray) -> "FunctionSpace":
    """The same space with dof d renamed new_of_old[d]; vectors move as x_new[new_of_old] = x_old."""
    return FunctionSpace(V.mesh, V.degree, np.ascontiguousarray(new_of_old[V.dofmap].astype(np.int32)), V.index_map, V.lattice,
                         structured=False)


def _int3(n):
    """three cell counts as the const int* of the wf_box_* entries"""
    return (ctypes.c_int * 3)(*(int(v) for v in n))


def create_box(n, lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0), perturb: float = 0.0, seed: int = 42) -> BoxMesh:
    """mesh::create_box(comm, {lo, hi}, {nx, ny, nz}, hexahedron) (wf_box_mesh).  perturb > 0
    displaces interior vertices by perturb*h*U(-1,1) (numpy default_rng(seed))."""
    if np.isscalar(n):
        n = (int(n),) * 3
    nx, ny, nz = (int(v) for v in n)
    x = np.empty(((nx + 1) * (ny + 1) * (nz + 1), 3))
    gd = np.empty((nx * ny * nz, 8), dtype=np.int32)
    corner = lambda c: np.array([float(v) for v in c])
    check(lib().wf_box_mesh(_int3((nx, ny, nz)), _dp(corner(lo)), _dp(corner(hi)), _dp(x), _ip(gd)))
    if perturb > 0.0:
        rng = np.random.default_rng(seed)
        h = np.array([(hi[0] - lo[0]) / nx, (hi[1] - lo[1]) / ny, (hi[2] - lo[2]) / nz])
        d = rng.uniform(-1.0, 1.0, size=x.shape) * (perturb * h)
        iz, iy, ix = np.meshgrid(np.arange(nz + 1), np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
        interior = ((ix > 0) & (ix < nx) & (iy > 0) & (iy < ny) & (iz > 0) & (iz < nz)).reshape(-1)
        x[interior] += d[interior]
    return BoxMesh((nx, ny, nz), x, gd, tuple(lo), tuple(hi))


def create_functionspace(mesh: BoxMesh, degree: int, build_dofmap: bool = True) -> FunctionSpace:
    """fem::create_functionspace(mesh, Lagrange(hexahedron, degree, gll_warped)) (wf_box_dofmap)."""
    nx, ny, nz = mesh.n
    p = int(degree)
    NX, NY, NZ = p * nx + 1, p * ny + 1, p * nz + 1
    dm = np.empty((nx * ny * nz if build_dofmap else 0, (p + 1) ** 3), dtype=np.int32)
    if build_dofmap:
        check(lib().wf_box_dofmap(p, _int3(mesh.n), _ip(dm)))
    return FunctionSpace(mesh, p, dm, IndexMap(NX * NY * NZ), (NX, NY, NZ))
