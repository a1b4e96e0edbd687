"""Helpers of the structured box stiffness tests, the owner-kernel family first: spaces on uniform and graded boxes,
operators, applies, inputs and the oracle's answer.  Imports without a GPU; torch is imported where it is used."""
import numpy as np

from support import lattice_x


def spaces(oracle, n, p, x=None, lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0), perturb=0.0):
    """(oracle mesh, FunctionSpace) of the box n; x replaces the vertex coordinates when given."""
    import wave_fenics_amd as w
    om = oracle.create_box(n, p, lo=lo, hi=hi, perturb=perturb)
    mesh = w.create_box(n, lo=lo, hi=hi, perturb=perturb)
    if x is not None:
        om.x = np.ascontiguousarray(x, dtype=np.float64)
        mesh = w.BoxMesh(mesh.n, om.x.copy(), mesh.geom_dofmap, lo, hi)
    assert np.array_equal(mesh.x, om.x)
    return om, w.create_functionspace(mesh, p)


def graded_axes(n, seed=11):
    rng = np.random.default_rng(seed)
    return [np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 2.0, m))]) for m in n]


def graded(oracle, n, p, seed=11):
    """spaces() on the rectilinear box whose cell widths are uniform in [0.5, 2) per axis."""
    return spaces(oracle, n, p, x=lattice_x(*graded_axes(n, seed)))


def stiffness(V, p, flags=0, **tuning):
    import wave_fenics_amd as w
    return w.StiffnessOperator(V, p, {"c0": 1500.0}, structured=True, flags=flags, tuning=tuning or None)


def owner(V, p, **tuning):
    """The owner form of the separable box operator, asserted to be that."""
    op = stiffness(V, p, update="owner", **tuning)
    assert (op.kernel, op.metric, op.update) == ("march_box", "axes", "owner")
    return op


def apply(op, x, y0, gpu):
    """y0 + A x on the host; x and y0 may be read-only."""
    import torch
    y = torch.from_numpy(y0.copy()).to(gpu)
    op(torch.from_numpy(np.array(x)).to(gpu), y)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def apply_from_zero(op, x, gpu):
    """A x on the host."""
    return apply(op, x, np.zeros(op.info.ndofs), gpu)


def inputs(om, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, om.ndofs), rng.uniform(-1, 1, om.ndofs) * 1e6


def reference(oracle, om, p, x, y0):
    y = y0.copy()
    oracle.StiffnessOperator(om, p)(x, y)
    return y


def owner_cut_candidates(nz):
    """The nseg of the tables that creation times against the uniform plan of a P4 owner operator (owner_cut_candidates,
    csrc/box_run_plan.cpp): runs of 4 to 12 layers, at most 17 candidates."""
    lo, hi = max(2, (nz + 11) // 12), nz // 4
    return list(range(lo, hi + 1, max(1, (hi - lo + 16) // 16)))


def aligned_runs(ncols, nz, nseg, nxcd=8):
    """aligned_runs of csrc/box_run_plan.cpp, restated: every column cut at layers nz s // nseg, the runs in segment-major
    order dealt to the XCDs in contiguous shares (the first n % 8 one run longer); run i of XCD xcd is entry 8 i + xcd.
    [runs][3] = (column, z0, z1), int32."""
    n = ncols * nseg
    start = np.concatenate([[0], np.cumsum(n // nxcd + (np.arange(nxcd) < n % nxcd))])
    t = np.arange(n)
    xcd = np.searchsorted(start, t, side="right") - 1
    s, col = t // ncols, t % ncols
    table = np.full((n, 3), -1, dtype=np.int32)
    table[nxcd * (t - start[xcd]) + xcd] = np.stack([col, nz * s // nseg, nz * (s + 1) // nseg], axis=1)
    return table


_boxes = {}


def box(oracle, n, p, seed, gpu=None):
    """One graded box: the space, x, a random non-zero y0 at the scale of K x, the oracle's y0 + K x and, with a gpu,
    the atomic form's y (None without).  Computed once per (n, p, seed) and read-only; the caller chooses the seed."""
    key = (n, p, seed, gpu is not None)
    if key not in _boxes:
        om, V = graded(oracle, n, p)
        rng = np.random.default_rng(seed)
        x = rng.uniform(-1, 1, om.ndofs)
        kx = np.zeros(om.ndofs)
        oracle.StiffnessOperator(om, p)(x, kx)
        y0 = rng.uniform(-1, 1, om.ndofs) * np.abs(kx).max()
        assert np.abs(y0).min() > 0.0
        yatom = None
        if gpu is not None:
            atom = stiffness(V, p, update="atomic")
            assert atom.update == "atomic"
            yatom = apply(atom, x, y0, gpu)
        _boxes[key] = (V, x, y0, y0 + kx, yatom)
        for a in _boxes[key][1:4 if yatom is None else 5]:
            a.setflags(write=False)
    return _boxes[key]
