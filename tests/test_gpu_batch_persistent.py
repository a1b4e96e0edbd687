"""The persistent loops of the hexahedral batch kernels (csrc/stiffness_batch.hip, csrc/mass_batch.hip) at several batches per workgroup.

A mesh that does not tile into lattice columns runs k_stiffness_generic_up2<P> (P1..P4), k_stiffness_generic_up<P>
(P5..P7) and, for the element-wise lumped mass, k_mass_lumped_u.  The stiffness launchers size their grid as
min(nbatch, per_cu * 256) with per_cu from an occupancy query, the mass launcher as min(nbatch, 2048); every other test
that selects these kernels has fewer batches than workgroups, so each workgroup runs one batch and the loops' carried
state is never used.  The meshes here are large enough that EVERY workgroup runs at least four batches whatever the
occupancy query returns.  The bound on the grid comes from the launch code alone:

    a 256-thread workgroup is 4 waves and a CU holds 32 waves               -> at most 8 workgroups per CU
    lds = (3 CB nd + n^2) 8 bytes, CB = 256 / n^2, nd = n^3, n = P + 1      -> at most floor(160 KiB / lds) per CU
    grid <= G_h = 256 min(8, floor(163840 / lds))

and nbatch >= 4 G_h + 1 does the rest.  nbatch % 256 != 0 (the grid is a multiple of 256) makes floor(nbatch / grid) and
ceil(nbatch / grid) both occur: odd and even trip counts of the loop unrolled by two, in one launch.  ncells % CB != 0
ends a multi-batch run with a partial batch.  test_sizes_reach_the_loops (no GPU needed) asserts all of it from these
formulas, for every grid that is a multiple of 256 up to G_h.

  case (box, cells)                       kernel                         what it reaches
  mixed P1 81x81x80, P2 62x61x61,         k_stiffness_generic_up2<P>     the A/B register sets (uq, x, g, lc) swapping roles;
        P3 47x46x46, P4 38x37x37                                         the rotation u0c,nuc <- u0n,nun <- u0nn,nunn <- u0n3,
                                                                         nun3 (a location loaded as b + 3s is the current one in
                                                                         a workgroup's fourth batch); both halves of the loop
                                                                         and both breaks; clampb() at the end of a run (the next
                                                                         batch is the last batch again, loaded and never stored)
  mixed P5 31x31x30, P6 27x24x24,         k_stiffness_generic_up<P>      uqa/uqb swapping roles, the indices fetched one batch
        P7 25x23x22                                                      ahead, `bn < nbatch ? bn : b` at the end of a run
  mixed, every degree                     both, k_mass_lumped_u          first half of the cell list lexicographic (compact
                                                                         batches, small nu: the `u < nu ? u : nu - 1` clamp is
                                                                         taken), second half shuffled (nu near CB nd): every
                                                                         workgroup starts in the first half and ends in the
                                                                         second, so nu changes inside every run; in
                                                                         k_mass_lumped_u the split Xu | Yu of the LDS tile moves
                                                                         with it; a partial last batch
  renumbered P2, P6                       one of each stiffness form     random global numbering, random element permutation
                                                                         (h_perm), the library's own cell sort
  whole P2, P5                            one of each stiffness form     the mixed list cut to a multiple of CB: a run that ends
                                                                         with a full batch
  plus_one P2, P5                         one of each stiffness form     that plus one cell: the last batch holds one cell.  The
                                                                         cut leaves dofs that no cell lists: x is NaN there and
                                                                         y starts from a sentinel that must come back bit for bit

k_mass_lumped_u's grid is exactly min(nbatch, 2048): two to five iterations of its grid-stride loop at P1..P5, a second
iteration in some workgroups at P6 and P7.  k_stiffness_generic<P> (tuning "elementwise": one batch per workgroup, no
loop, a scatter of its own) runs on the same space as a second implementation of the same sum.

References.  Stiffness: oracle.stiffness_apply_sumfact (float64 C) with oracle.precompute_geometric_data, on the box in
its own lexicographic dof numbering and ascending cell order (cells that a case drops are left out), mapped through the
case's permutations.  tests/test_oracle_kat.py::test_dense_equals_sumfact pins it to the dense restatement at small
sizes; test_reference_slice (no GPU needed) repeats that on 64 cells of every case's mesh, at these cell sizes.  Lumped
mass: oracle.MassOperatorCPU.  Tolerances are the project's own: kernel against oracle max|y - y_ref| <= 1e-12 max|K x|
(SURVEY 8c / BASELINE.json), mass 1e-13 max|M x|, batch against element-wise and an apply against its repeat 1e-13
(another order of the same atomics).  y starts from uniform(-1, 1) max|K x|, so that neither the start nor the increment
hides the other (at h = 1/80 the increment is far below the 1e6 the small tests start from).  Every measured error is
printed.

One case at a time is kept alive (its reference-layout G is 0.3 to 0.5 GB on the host)."""
import functools
import time
from dataclasses import dataclass

import numpy as np
import pytest

from support import cells_per_batch, gpu  # noqa: F401

gpu_test = pytest.mark.gpu

C0 = 1500.0
TOL = 1e-12                       # kernel against the float64 oracle, of max|K x|
TOL_MASS = 1e-13
TOL_FORM = 1e-13                  # two forms, or two runs, of the same sum
LDS_PER_CU = 160 * 1024
WAVES_PER_CU, WAVES_PER_WORKGROUP = 32, 4
MASS_GRID = 256 * 8               # launch_mass_lumped_u
SENTINEL = -7.0e77
SLICE = 64                        # cells of test_reference_slice

BOXES = {1: (81, 81, 80), 2: (62, 61, 61), 3: (47, 46, 46), 4: (38, 37, 37), 5: (31, 31, 30), 6: (27, 24, 24),
         7: (25, 23, 22)}
CASES = ([("mixed", p) for p in range(1, 8)] + [("renumbered", 2), ("renumbered", 6)]
         + [("whole", 2), ("plus_one", 2), ("whole", 5), ("plus_one", 5)])
case_params = pytest.mark.parametrize("kind,p", CASES, ids=[f"{k}_P{p}" for k, p in CASES])


def lds_bytes(p):
    """dynamic LDS of k_stiffness_generic_up / _up2: U, Fr, Fs [CB][nd] and the n x n derivative table"""
    n = p + 1
    return (3 * cells_per_batch(p) * n ** 3 + n * n) * 8


def grid_bound(p):
    """no occupancy query can return more workgroups per CU than the waves or the LDS of a CU allow"""
    return 256 * min(WAVES_PER_CU // WAVES_PER_WORKGROUP, LDS_PER_CU // lds_bytes(p))


def batch_unique(dm, cb):
    """unique dofs of every batch of cb cells in the order of dm, as build_unique_lists counts them"""
    return np.array([np.unique(dm[b:b + cb]).size for b in range(0, dm.shape[0], cb)])


@dataclass
class Case:
    kind: str
    p: int
    om: object                    # the box in its own numbering (oracle.BoxMesh)
    cells: np.ndarray             # the case's cell list: cells of om, in the order the library is given
    gperm: np.ndarray             # dof d of om is dof gperm[d] of the case (None: the same)
    eperm: np.ndarray             # tensor -> element order (None: tensor order)
    keep: bool                    # wf_tuning.keep_cell_order

    @property
    def ncells(self):
        return int(self.cells.size)

    @property
    def nbatch(self):
        cb = cells_per_batch(self.p)
        return (self.ncells + cb - 1) // cb

    def tensor_dofmap(self):
        """the case's dofmap in its cell order and numbering, local dofs in tensor order"""
        dm = self.om.dofmap[self.cells]
        return dm if self.gperm is None else self.gperm[dm]

    def dofmap(self):
        """what the library is handed: element order"""
        dm = self.tensor_dofmap()
        if self.eperm is not None:
            inv = np.empty_like(self.eperm)
            inv[self.eperm] = np.arange(self.eperm.size, dtype=np.int32)
            dm = dm[:, inv]
        return np.ascontiguousarray(dm, dtype=np.int32)

    def reference_mesh(self, oracle):
        """om without the cells the case drops, ascending"""
        om = self.om
        if self.ncells == om.ncells:
            return om
        kept = np.sort(self.cells)
        return oracle.BoxMesh(om.n, om.p, om.x, np.ascontiguousarray(om.geom_dofmap[kept]),
                              np.ascontiguousarray(om.dofmap[kept]), om.ndofs, om.lattice)

    def listed(self):
        """dofs of om that some cell of the case lists"""
        m = np.zeros(self.om.ndofs, dtype=bool)
        m[self.om.dofmap[self.cells].reshape(-1)] = True
        return m

    def to_case(self, v):
        """a vector in om's numbering -> the case's numbering"""
        if self.gperm is None:
            return v
        out = np.empty_like(v)
        out[self.gperm] = v
        return out

    def from_case(self, v):
        return v if self.gperm is None else v[self.gperm]


@functools.lru_cache(maxsize=1)
def make_case(kind, p):
    from oracle import wave_oracle as oracle
    om = oracle.create_box(BOXES[p], p, perturb=0.2)
    rng = np.random.default_rng(1000 * p + len(kind))
    cb = cells_per_batch(p)
    if kind == "renumbered":
        gperm = rng.permutation(om.ndofs).astype(np.int32)
        eperm = rng.permutation((p + 1) ** 3).astype(np.int32)
        return Case(kind, p, om, np.arange(om.ncells), gperm, eperm, False)
    half = om.ncells // 2
    cells = np.concatenate([np.arange(half), half + rng.permutation(om.ncells - half)])
    if kind != "mixed":
        cells = cells[:om.ncells // cb * cb + (kind == "plus_one")]
    return Case(kind, p, om, cells, None, None, True)


# ---------------------------------------------------------------------------------------------------------------------
# no GPU needed: the cases are what the header says, the reference is sound at these sizes
# ---------------------------------------------------------------------------------------------------------------------
@case_params
def test_sizes_reach_the_loops(kind, p):
    case = make_case(kind, p)
    n = p + 1
    cb, nd, nb, gh = cells_per_batch(p), n ** 3, case.nbatch, grid_bound(p)
    assert cb * n * n <= 256 and (cb + 1) * n * n > 256
    assert lds_bytes(p) <= 64 * 1024 and gh % 256 == 0 and 256 <= gh <= 2048
    # every workgroup runs at least four batches, and both trip counts occur, at every grid the launcher can choose
    assert nb >= 4 * gh + 1
    assert nb % 256 != 0
    for grid in range(256, gh + 1, 256):
        assert nb // grid >= 4 and nb % grid != 0
    # k_mass_lumped_u: a second iteration of the grid-stride loop
    assert nb > MASS_GRID
    # the last batch
    if kind in ("mixed", "renumbered"):
        assert case.ncells % cb != 0 and case.ncells == case.om.ncells
    else:
        assert case.ncells % cb == (1 if kind == "plus_one" else 0) and case.om.ncells - cb < case.ncells < case.om.ncells
    print(f"{kind} P{p}: ncells {case.ncells} CB {cb} nbatch {nb} G_h {gh} lds {lds_bytes(p)} "
          f"batches per workgroup >= {nb // gh}, last batch {case.ncells - (nb - 1) * cb} cells")
    if kind == "renumbered":
        assert np.array_equal(np.sort(case.gperm), np.arange(case.om.ndofs))
        return
    # compact batches first, scattered batches last: a workgroup's first batch is one of the first `grid`, its last full
    # batch one of the last `grid` before the final one
    nu = batch_unique(case.tensor_dofmap(), cb)
    assert nu.size == nb
    assert np.median(nu[nb // 2 + 1:]) > np.median(nu[:nb // 2])
    assert nu[:gh].max() < nu[nb - 1 - gh:nb - 1].min()
    assert nu[:gh].max() < 256 * ((cb * nd + 255) // 256)      # register slots past the list: the clamp is taken
    assert nu.max() <= cb * nd
    print(f"   nu: first half median {int(np.median(nu[:nb // 2]))} max {nu[:nb // 2].max()}, second half median "
          f"{int(np.median(nu[nb // 2 + 1:]))} min {nu[nb // 2 + 1:nb - 1].min()}, last batch {nu[-1]}")
    unlisted = int((~case.listed()).sum())
    assert (unlisted > 0) == (kind in ("whole", "plus_one"))


@case_params
def test_reference_slice(oracle, kind, p):
    """The sum-factorised reference against the dense restatement of the reference operator on 64 cells of the case's
    mesh (the first of its shuffled half), through the cells= range of both."""
    case = make_case(kind, p)
    om = case.om
    half = case.ncells // 2
    win = case.cells[half - SLICE:half + 2 * SLICE]
    sub = oracle.BoxMesh(om.n, p, om.x, np.ascontiguousarray(om.geom_dofmap[win]), np.ascontiguousarray(om.dofmap[win]),
                         om.ndofs, om.lattice)
    K = oracle.StiffnessOperator(sub, p, {"c0": C0})
    x = np.random.default_rng(p).uniform(-1, 1, om.ndofs)
    y1, y2 = np.zeros(om.ndofs), np.zeros(om.ndofs)
    K(x, y1, cells=(SLICE, 2 * SLICE))
    oracle.stiffness_apply_sumfact(sub, K.G, C0, x, y2, cells=(SLICE, 2 * SLICE))
    touched = np.zeros(om.ndofs, dtype=bool)
    touched[sub.dofmap[SLICE:2 * SLICE].reshape(-1)] = True
    assert np.all(y2[~touched] == 0.0) and np.all(y1[~touched] == 0.0) and np.abs(y1).max() > 0.0
    err = np.abs(y1 - y2).max() / np.abs(y1).max()
    print(f"{kind} P{p}: sum-factorised against dense on {SLICE} cells {err:.2e}")
    assert err <= 1e-14
    with pytest.raises(ValueError):
        oracle.stiffness_apply_sumfact(sub, K.G, C0, x, y2, cells=(0, sub.ncells + 1))


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------


def apply_twice(op, x, y0, gpu):
    """y0 + A x, twice, each into a fresh copy of y0"""
    import torch
    xd = torch.from_numpy(x).to(gpu)
    out = []
    for _ in range(2):
        y = torch.from_numpy(y0).to(gpu)
        op(xd, y)
        out.append(y.cpu().numpy())
    return out


def check_untouched(y, listed, what):
    """finite wherever a cell lists the dof, the sentinel bit for bit wherever none does"""
    assert np.isfinite(y[listed]).all(), what
    assert np.array_equal(y[~listed].view(np.int64), np.full(int((~listed).sum()), SENTINEL).view(np.int64)), what


@gpu_test
@case_params
def test_batch_kernels_many_batches_per_workgroup(gpu, oracle, kind, p):
    import wave_fenics_amd as w
    from wave_fenics_amd._lib import WF_FLAG_MASS_ELEMENTWISE
    t0 = time.time()
    case = make_case(kind, p)
    om = case.om
    listed = case.listed()
    rng = np.random.default_rng(7 * p + len(kind))
    x = rng.uniform(-1, 1, om.ndofs)
    x[~listed] = np.nan
    start = rng.uniform(-1, 1, om.ndofs)

    # references: K x and M x on their own, then y0 = uniform * max|.| and y_ref = y0 + (.)
    ref = case.reference_mesh(oracle)
    M = oracle.MassOperatorCPU(ref, p)
    kx, mx = np.zeros(om.ndofs), np.zeros(om.ndofs)
    oracle.stiffness_apply_sumfact(ref, M.G, C0, x, kx)
    M(x, mx)
    del M, ref
    assert np.isfinite(kx).all() and np.isfinite(mx).all()              # the references read no unlisted dof either
    assert not kx[~listed].any() and not mx[~listed].any()
    sk, sm = np.abs(kx).max(), np.abs(mx).max()
    yk0, ym0 = start * sk, start * sm
    yk0[~listed] = ym0[~listed] = SENTINEL
    ykref, ymref = yk0 + kx, ym0 + mx
    t1 = time.time()

    mesh = w.BoxMesh(om.n, om.x, np.ascontiguousarray(om.geom_dofmap[case.cells]))
    V = w.FunctionSpace(mesh, p, case.dofmap(), w.IndexMap(om.ndofs), om.lattice, structured=False)
    xc = case.to_case(x)
    listed_c = case.to_case(listed)

    def run(op, y0, yref, scale, tol, what):
        ys = apply_twice(op, xc, case.to_case(y0), gpu)
        for y in ys:
            check_untouched(y, listed_c, what)
        ys = [case.from_case(y) for y in ys]
        errs = [np.abs(y - yref).max() / scale for y in ys]
        rep = np.abs(ys[0] - ys[1]).max() / scale
        print(f"{kind} P{p} {what}: against the oracle {errs[0]:.2e} {errs[1]:.2e}, repeat {rep:.2e}")
        assert max(errs) <= tol, (kind, p, what, errs)
        assert rep <= TOL_FORM, (kind, p, what, rep)
        return ys[0]

    op = w.StiffnessOperator(V, p, {"c0": C0}, perm=case.eperm, structured=False,
                             tuning={"kernel": "batch", "keep_cell_order": case.keep})
    assert op.kernel == "batch_unique" and op.num_cells() == case.ncells
    yb = run(op, yk0, ykref, sk, TOL, "stiffness batch")
    op.close()
    op = w.StiffnessOperator(V, p, {"c0": C0}, perm=case.eperm, structured=False,
                             tuning={"kernel": "elementwise", "keep_cell_order": True})
    assert op.kernel == "elementwise"
    ye = run(op, yk0, ykref, sk, TOL, "stiffness element-wise")
    op.close()
    form = np.abs(yb - ye).max() / sk
    print(f"{kind} P{p} stiffness batch against element-wise {form:.2e}")
    assert form <= TOL_FORM, (kind, p, form)
    op = w.MassOperatorLumped(V, p, perm=case.eperm, structured=False, flags=WF_FLAG_MASS_ELEMENTWISE,
                              tuning={"kernel": "batch", "keep_cell_order": case.keep})
    assert op.kernel == "batch_unique"
    run(op, ym0, ymref, sm, TOL_MASS, "lumped mass batch")
    op.close()
    print(f"{kind} P{p}: {case.ncells} cells, {case.nbatch} batches, reference {t1 - t0:.1f} s, GPU side "
          f"{time.time() - t1:.1f} s")
