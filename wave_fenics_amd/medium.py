"""Heterogeneous media: sound speed and density per cell, and the cell coefficients the operators take.

The model is (1 / (rho c^2)) p_tt = div((1 / rho) grad p): tissue, fat and bone differ in both c and rho.  A Medium
holds one value of each per cell, in the mesh's cell order (the rows of mesh.geom_dofmap; on a box
cx + nx (cy + ny cz)), and derives what the operators of this package take as cell_coeff=:

    mass_coeff  = 1 / (rho c^2)   lumped (or dense) mass
    stiff_coeff = 1 / rho         stiffness, created with c0 = 1
    admittance  = 1 / (rho c)     weight of the facet masses of both boundary terms

LinearGLLOpt(..., medium=Medium(c, rho)) assembles the model from them.  A coefficient is constant in a cell; a
medium cannot be changed once the operators exist."""
from __future__ import annotations

import numpy as np

from .mesh_io import whole_steps


class Medium:
    """Medium(c, rho=None): sound speed and density per cell ([ncells] each; rho = None is rho = 1).  Both must be
    finite and positive."""

    def __init__(self, c, rho=None):
        self.c = np.ascontiguousarray(c, dtype=np.float64).reshape(-1)
        self.rho = np.ones_like(self.c) if rho is None else np.ascontiguousarray(rho, dtype=np.float64).reshape(-1)
        if self.rho.shape != self.c.shape:
            raise ValueError(f"Medium: c has {self.c.size} cells, rho has {self.rho.size}")
        for name, a in (("c", self.c), ("rho", self.rho)):
            bad = np.nonzero(~(np.isfinite(a) & (a > 0.0)))[0]
            if bad.size:
                raise ValueError(f"Medium: {name}[{bad[0]}] = {a[bad[0]]} is not a finite positive value")

    @property
    def ncells(self) -> int:
        return int(self.c.size)

    @property
    def mass_coeff(self) -> np.ndarray:
        return 1.0 / (self.rho * self.c ** 2)

    @property
    def stiff_coeff(self) -> np.ndarray:
        return 1.0 / self.rho

    @property
    def admittance(self) -> np.ndarray:
        return 1.0 / (self.rho * self.c)

    @classmethod
    def from_centroids(cls, mesh, fn) -> "Medium":
        """The medium whose cell values are fn at the cell centroids (mean of the cell's vertices): fn takes an
        array [ncells][3] and returns c [ncells], or the pair (c, rho)."""
        xc = np.asarray(mesh.x)[np.asarray(mesh.geom_dofmap)].mean(axis=1)
        out = fn(xc)
        if isinstance(out, tuple):
            return cls(*out)
        return cls(out)


def cell_diameters(mesh) -> np.ndarray:
    """mesh::h per cell: the largest distance between two of its vertices (demo/cpu_planar3d/main.cpp:48-57)."""
    xc = np.asarray(mesh.x)[np.asarray(mesh.geom_dofmap)]
    d = np.linalg.norm(xc[:, :, None, :] - xc[:, None, :, :], axis=3)
    return d.reshape(d.shape[0], -1).max(axis=1)


def cfl_time_step(mesh, degree: int, medium: Medium, freq: float, CFL: float = 0.5):
    """The time step of demo/cpu_planar3d/main.cpp:48-66 in a heterogeneous medium: dt = CFL min_c(h_c / c_c) / P^2,
    rounded to whole steps per period as linear_gll.cfl_time_step does.  The limiting cell is the one a wave crosses
    fastest, which need be neither the smallest nor the one with the highest speed.  Returns (dt, steps per period)."""
    if medium.ncells != mesh.ncells:
        raise ValueError(f"medium has {medium.ncells} cells, the mesh has {mesh.ncells}")
    # per cell the expression of the homogeneous function, so that a uniform medium gives its dt bit for bit
    dt = (CFL * cell_diameters(mesh) / (medium.c * degree ** 2)).min()
    return whole_steps(dt, freq)
