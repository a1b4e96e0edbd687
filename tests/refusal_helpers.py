"""The refusals of the four creation entry points built on the operator descriptor -- wf_op_create,
wf_op_create_box_coeff, wf_cell_form_create, wf_cell_form_create_box -- as a table of (entry, case, return code,
wf_last_error text), and the generator of tests/golden/refusal_table.json (tests/test_refusal_table.py replays it).

Every case is a descriptor with one defect or two, at P2 on the 2 x 1 x 1 box; with two defects the order of the
library's checks decides which one is reported, and the table pins that order.  Every refusal listed here precedes the
first device call, so the table is the same on a machine with a GPU and on one without.  No tests and no GPU in here.

    python tests/refusal_helpers.py        writes the fixture from the library in the tree"""
from __future__ import annotations

import ctypes
import itertools
import json
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusal_table.json")
INVALID, UNSUPPORTED = -1, -2
P, BOX = 2, (2, 1, 1)
# the defects every pair is taken from, in the order in which two of them are applied
PAIRED = ("degree8", "kind_unknown", "negative_size", "null_dofmap", "dofmap_range", "bad_perm", "vertex_minus1",
          "nan_coeff", "stray_tuning", "stray_flag")
BOX_ONLY = ("null_xverts", "lattice_2p31")
# defects that describe no array of a box entry point
DESC_ONLY = ("null_dofmap", "dofmap_range", "bad_perm", "vertex_minus1")
TUNING_FIELDS = ("kernel", "variant", "lz", "lz0", "bx", "by", "bz", "keep_cell_order", "orient", "metric", "update")


class Case:
    """The arguments of one call: the descriptor of the dofmap entry points and the argument list of the box ones,
    with the arrays both point into."""

    def __init__(self, wlib, p=P, n=BOX, perturb=0.0):
        import wave_fenics_amd as w
        self.wlib = wlib
        mesh = w.create_box(n, perturb=perturb)
        V = w.create_functionspace(mesh, p)
        self.dofmap = np.ascontiguousarray(V.dofmap, dtype=np.int32)
        self.x = np.ascontiguousarray(mesh.x, dtype=np.float64)
        self.geom = np.ascontiguousarray(mesh.geom_dofmap, dtype=np.int32)
        self.kind, self.degree, self.n = wlib.WF_OP_STIFFNESS, p, list(n)
        self.ncells, self.ndofs = mesh.ncells, V.ndofs
        self.have_dofmap = self.have_x = self.have_mesh = True
        self.perm = self.coeff = self.G = None
        self.flags = 0
        self.tuning = None
        self.null_desc = self.null_out = False

    def tune(self, **fields):
        self.tuning = self.tuning or self.wlib.Tuning()
        for k, v in fields.items():
            setattr(self.tuning, k, v)

    def apply(self, defect: str):
        wlib = self.wlib
        if defect == "degree8":
            self.degree = 8
        elif defect == "kind_unknown":
            self.kind = 7
        elif defect == "kind_dense":
            self.kind = wlib.WF_OP_MASS_DENSE
        elif defect == "kind_lumped":              # no defect: the lumped mass in the place of the stiffness operator
            self.kind = wlib.WF_OP_MASS_LUMPED
        elif defect == "negative_size":
            self.ncells, self.n[0] = -1, -1
        elif defect == "null_dofmap":
            self.have_dofmap = False
        elif defect == "dofmap_range":
            self.dofmap[1, 3] = self.ndofs
        elif defect == "bad_perm":
            self.perm = np.arange((self.degree + 1) ** 3 if self.degree <= 7 else 27, dtype=np.int32)
            self.perm[5] = 4
        elif defect == "vertex_minus1":
            self.geom[0, 0] = -1
        elif defect == "nan_coeff":
            self.coeff = np.array([1.0, float("nan")])
        elif defect == "stray_tuning":
            self.tune(kernel=wlib.WF_KERNEL_FORCE_MASS_MARCH)
        elif defect == "stray_flag":
            self.flags |= wlib.WF_FLAG_ORDERED
        elif defect == "flag_elementwise":
            self.flags |= wlib.WF_FLAG_MASS_ELEMENTWISE
        elif defect == "null_xverts":
            self.have_x = False
        elif defect == "lattice_2p31":
            self.n[2] = 1 << 30
        elif defect == "with_G":
            self.G = np.zeros((self.ncells, (self.degree + 1) ** 3, 3, 3))
            self.have_mesh = False
        elif defect == "no_mesh":
            self.have_mesh = False
        elif defect == "null_desc":
            self.null_desc = True
        elif defect == "null_out":
            self.null_out = True
        elif defect.startswith("tuning."):          # tuning.<field>=<value>
            field, value = defect[len("tuning."):].split("=")
            self.tune(**{field: int(value)})
        else:
            raise KeyError(defect)

    def desc(self):
        wlib = self.wlib
        d = wlib.OpDesc()
        d.kind, d.degree, d.ncells, d.ndofs = self.kind, self.degree, self.ncells, self.ndofs
        d.c0 = 1500.0
        d.flags = self.flags
        if self.have_dofmap:
            d.h_dofmap = wlib._ip(self.dofmap)
        d.h_perm = wlib._ip(self.perm)
        d.h_G = wlib._dp(self.G)
        if self.have_mesh:
            d.nverts = self.x.shape[0]
            d.h_geom_dofmap = wlib._ip(self.geom)
            if self.have_x:
                d.h_xverts = wlib._dp(self.x)
        d.h_cell_coeff = wlib._dp(self.coeff)
        if self.tuning is not None:
            d.tuning = ctypes.pointer(self.tuning)
        return d

    def call(self, entry: str):
        """(return code, wf_last_error text); a handle that was made after all is destroyed"""
        wlib = self.wlib
        L = wlib.lib()
        h = ctypes.c_void_p()
        out = None if self.null_out else ctypes.byref(h)
        if entry in ("wf_op_create", "wf_cell_form_create"):
            d = self.desc()
            rc = getattr(L, entry)(None if self.null_desc else ctypes.byref(d), out)
        else:
            nx, ny, nz = self.n
            t = ctypes.byref(self.tuning) if self.tuning is not None else None
            rc = getattr(L, entry)(self.kind, self.degree, nx, ny, nz, wlib._dp(self.x) if self.have_x else None, 1500.0,
                                   wlib._dp(self.coeff), self.flags, t, out)
        if h.value:
            (L.wf_op_destroy if entry.startswith("wf_op") else L.wf_cell_form_destroy)(h)
        return rc, L.wf_last_error().decode()


# the single defects of every entry point: those tests/test_cell_form_host.py::test_refusals_before_any_device_call
# lists, where the entry point refuses them on the host (wf_op_create accepts a flag or a tuning field that the cell
# form refuses, and goes on to the device), and the host checks around the per-cell request
SINGLES = {
    "wf_cell_form_create":
        ["kind_dense", "stray_flag", "kind_lumped+stray_flag", "flag_elementwise", "kind_lumped+flag_elementwise"]
        + [f"tuning.{f}=1" for f in TUNING_FIELDS]
        + ["tuning.geometry=3", "with_G+tuning.geometry=2", "nan_coeff", "null_desc", "null_out", "null_dofmap", "null_xverts",
           "kind_lumped+null_xverts", "dofmap_range", "vertex_minus1", "degree8", "kind_unknown", "negative_size", "bad_perm",
           "stray_tuning"],
    "wf_op_create":
        ["nan_coeff", "null_desc", "null_out", "null_dofmap", "null_xverts", "dofmap_range", "vertex_minus1", "degree8",
         "kind_unknown", "negative_size", "bad_perm", "stray_tuning", "with_G+tuning.geometry=2", "no_mesh+tuning.geometry=2",
         "tuning.geometry=2+tuning.kernel=1", "tuning.geometry=2+tuning.update=3", "tuning.geometry=2+tuning.update=2",
         "tuning.geometry=2+tuning.metric=3"],
    "wf_op_create_box_coeff":
        ["null_xverts", "kind_dense", "kind_unknown", "degree8", "negative_size", "nan_coeff", "stray_tuning", "null_out",
         "lattice_2p31", "tuning.geometry=3", "tuning.metric=3", "tuning.update=3"],
    "wf_cell_form_create_box":
        ["null_xverts", "kind_dense", "kind_unknown", "degree8", "negative_size", "nan_coeff", "stray_tuning", "stray_flag",
         "flag_elementwise", "null_out", "lattice_2p31", "tuning.geometry=3", "tuning.lz=1"],
}


def cases(entry: str):
    """the case names of an entry point: its singles, then every pair"""
    box = entry.endswith("_box") or entry.endswith("_box_coeff")
    pool = [d for d in PAIRED if not (box and d in DESC_ONLY)] + (list(BOX_ONLY) if box else [])
    return SINGLES[entry] + [f"{a}+{b}" for a, b in itertools.combinations(pool, 2)]


def per_cell_refusal(wlib, entry: str):
    """WF_GEOMETRY_PER_CELL on the perturbed 3 x 3 x 3 box at P2"""
    c = Case(wlib, 2, (3, 3, 3), perturb=0.2)
    c.tune(geometry=2)
    return c.call(entry)


def record(wlib):
    """the table, from the library that is loaded"""
    rows = []
    for entry in SINGLES:
        for name in cases(entry):
            c = Case(wlib)
            for defect in name.split("+"):
                c.apply(defect)
            rc, msg = c.call(entry)
            rows.append({"entry": entry, "case": name, "rc": rc, "msg": msg})
    for entry in ("wf_op_create", "wf_cell_form_create"):
        rc, msg = per_cell_refusal(wlib, entry)
        rows.append({"entry": entry, "case": "per_cell on the perturbed 3x3x3 box", "rc": rc, "msg": msg})
    return rows


def write_fixture(wlib, path: str = FIXTURE):
    rows = record(wlib)
    bad = [r for r in rows if r["rc"] not in (INVALID, UNSUPPORTED)]
    assert not bad, f"not refused on the host: {bad}"
    with open(path, "w") as f:
        json.dump(rows, f, indent=0)
        f.write("\n")
    return rows


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from support import built_lib
    print(len(write_fixture(built_lib())), "rows ->", FIXTURE)
