"""Per-cell geometry of the dofmap stiffness operator: wf_tuning.geometry = WF_GEOMETRY_PER_CELL on wf_op_create
(StiffnessOperator(..., structured=False, tuning={"geometry": "per_cell"})), degrees 1 to 4, on the lattice-column plan
-- k_march_idx<P, BX, BY, cell | cell_axes> (csrc/stiffness_march_idx.hip) reading one G_c per cell in the plan's frame.

Every per-cell operator is checked against the CPU oracle (1e-12 of max|y_ref|) and against the per-point operator on
the same mesh and tuning (1e-13: the two differ only in how G is rounded), with y0 random at the scale of K x, and
asserts kernel == "march_idx" and geometry == "per_cell": a silent fall-back to the per-point kernel cannot pass.  The
meshes (tests/idx_cell_helpers.py) are shown affine, and the rectilinear ones diagonal, by tests/test_idx_cell_host.py."""
import os
import subprocess

import numpy as np
import pytest

import idx_cell_helpers as h
from nonbox_helpers import STIFFNESS_BLOCK
from support import dev, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_ORACLE = 1e-12
TOL_POINT = 1e-13
C0 = {"c0": 1500.0}


def stiffness(V, p, flags=0, **tuning):
    import wave_fenics_amd as w
    return w.StiffnessOperator(V, p, C0, structured=False, flags=flags, tuning=tuning or None)


def run(op, ref, gpu):
    y = dev(ref.y0, gpu)
    op(dev(ref.x, gpu), y)
    return y.cpu().numpy()


def check_pair(V, p, ref, gpu, expect, flags=0, **tuning):
    """The per-cell operator (of the expected metric) and the per-point one with the same tuning, both against the
    oracle and against each other.  Returns the two operators.  (Without the request a plan with a low fill -- a small
    mesh in a wide cross-section -- keeps the batch kernel: the per-point operator is whichever kernel creation picks.)"""
    pc = stiffness(V, p, flags, geometry="per_cell", **tuning)
    pp = stiffness(V, p, flags, **tuning)
    assert (pc.kernel, pc.geometry, pc.metric) == ("march_idx", "per_cell", expect), (pc.kernel, pc.geometry, pc.metric)
    assert pc.update == ("atomic" if expect == "axes" else "none")
    assert pp.kernel in ("march_idx", "batch_unique") and (pp.geometry, pp.metric) == ("per_point", "none")
    y, ypp = run(pc, ref, gpu), run(pp, ref, gpu)
    e_or, e_pp, e_pt = np.abs(y - ref.yref).max() / ref.scale, np.abs(ypp - ref.yref).max() / ref.scale, np.abs(y - ypp).max() / ref.scale
    print(f"P{p} {expect}: per-cell vs oracle {e_or:.2e}, per-point vs oracle {e_pp:.2e}, per-cell vs per-point {e_pt:.2e}")
    assert e_or <= TOL_ORACLE and e_pp <= TOL_ORACLE, (e_or, e_pp)
    assert e_pt <= TOL_POINT, e_pt
    return pc, pp


# ---- 1. parity across meshes ----
@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("name", h.PARITY_MESHES)
def test_parity_across_meshes(gpu, oracle, name, p):
    V, ref = h.space(name, p), h.reference(name, p)
    metric = "axes" if h.is_rectilinear(name) else "full"
    pc, pp = check_pair(V, p, ref, gpu, metric)
    turned = name.endswith("-random") or name.startswith("glued")
    assert (pc.info.plan_reoriented > 0) == turned
    if name == "anisotropic-random":   # the full form forced on a rectilinear mesh
        check_pair(V, p, ref, gpu, "full", metric="full")


# ---- 2. the layer loop ----
@pytest.mark.parametrize("lz", [1, 2, 3, 4, 0])
@pytest.mark.parametrize("p", [2, 4])
def test_layer_loop(gpu, oracle, p, lz):
    """(6, 3, 7): items of 1, 2, 3 and 4 layers -- both halves of the loop unrolled by two, the On / Off copies of the
    layer body at P4, a short last item -- and the plan's own choice (lz = 0), in both forms."""
    V, ref = h.space("column-7", p), h.reference("column-7", p)
    for metric in ("axes", "full"):
        pc, _ = check_pair(V, p, ref, gpu, metric, lz=lz, metric=metric)
        if lz:
            bx, by = STIFFNESS_BLOCK[p]
            assert pc.info.plan_lz == lz and pc.info.plan_items == -(-7 // lz) * -(-6 // bx) * -(-3 // by)


# ---- 3. holes ----
@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("name", h.HOLED)
def test_holed_meshes(gpu, oracle, name, p):
    """Empty slots carry a zero G_c; the stair has work items whose first layer is empty.  The plan is adopted whatever
    its fill."""
    V, ref = h.space(name, p), h.reference(name, p)
    pc, _ = check_pair(V, p, ref, gpu, "axes", kernel="march")
    assert 0.0 < pc.info.plan_fill < 1.0
    check_pair(V, p, ref, gpu, "full", kernel="march", metric="full", lz=2)
    assert stiffness(V, p, geometry="per_cell").kernel == "march_idx"   # no fill threshold for the request


# ---- 4. flags ----
@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("name", ["glued_reflected", "glued_mirrored", "sheared-random"])
def test_flags(gpu, oracle, name, p):
    """WF_FLAG_NO_CLAMP changes nothing on these meshes (the request is only granted where the clamp has no effect);
    WF_FLAG_NO_FABS keeps the sign of det J: on glued_mirrored block 2 is a true reflection and enters negated (the
    oracle takes |det J|: its reference applies the two blocks separately)."""
    from wave_fenics_amd._lib import WF_FLAG_NO_CLAMP, WF_FLAG_NO_FABS
    V = h.space(name, p)
    metric = "axes" if h.is_rectilinear(name) else "full"
    for flags in (0, WF_FLAG_NO_CLAMP, WF_FLAG_NO_FABS, WF_FLAG_NO_FABS | WF_FLAG_NO_CLAMP):
        ref = h.reference(name, p, bool(flags & WF_FLAG_NO_FABS))
        if name == "glued_mirrored" and flags & WF_FLAG_NO_FABS:
            assert ref.nneg == 48
            assert np.abs(ref.yref - h.reference(name, p).yref).max() > 1e-3 * ref.scale   # the flag matters here
        check_pair(V, p, ref, gpu, metric, flags=flags)


# ---- 5. parts ----
@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("metric", ["axes", "full"])
def test_parts_sum_to_the_full_apply(gpu, oracle, p, metric):
    import torch
    from wave_fenics_amd._lib import WF_PART_INTERFACE, WF_PART_INTERIOR, WF_PART_INTERIOR_A, WF_PART_INTERIOR_B
    name = "column-7"
    V, ref = h.space(name, p), h.reference(name, p)
    op = stiffness(V, p, geometry="per_cell", metric=metric, lz=2)
    assert (op.kernel, op.geometry, op.metric) == ("march_idx", "per_cell", metric)
    X = V.dof_coordinates
    ghosts = np.nonzero((X[:, 2] == X[:, 2].min()) | (X[:, 2] == X[:, 2].max()))[0]   # the dofs of two faces
    assert op.set_ghost_dofs(ghosts)
    assert op.info.items_interior > 0 and op.info.items_interface > 0
    x = dev(ref.x, gpu)
    yfull = run(op, ref, gpu)
    for parts in ((WF_PART_INTERIOR, WF_PART_INTERFACE), (WF_PART_INTERIOR_A, WF_PART_INTERFACE, WF_PART_INTERIOR_B)):
        y = dev(ref.y0, gpu)
        for part in parts:
            op.apply_part(x, y, part)
        torch.cuda.synchronize()
        assert np.abs(y.cpu().numpy() - yfull).max() <= TOL_POINT * ref.scale, parts
    assert np.abs(yfull - ref.yref).max() <= TOL_ORACLE * ref.scale


# ---- 6. info ----
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_info(gpu, p):
    """alg_bytes by the per-cell formula; device_bytes without the per-point stream: exactly 48 B instead of 48 nd B per
    cell slot of the plan (and n^2 + n more table entries: the weights and A).  The bound of the box test,
    device_bytes < 2 (per-point device_bytes) / nd, holds where the index tables are shared by many work items -- the
    box has none: a column of 12 layers cut into items of one layer."""
    n, nd = p + 1, (p + 1) ** 3
    bx, by = STIFFNESS_BLOCK[p]
    for name, lz in (("graded-random", 0), ("column-12", 1)):
        V = h.space(name, p)
        for metric in ("axes", "full"):
            pc = stiffness(V, p, geometry="per_cell", metric=metric, lz=lz)
            pp = stiffness(V, p, kernel="march", lz=lz)
            assert (pc.kernel, pc.geometry, pc.metric) == ("march_idx", "per_cell", metric)
            assert (pp.kernel, pp.geometry) == ("march_idx", "per_point")
            assert pc.alg_bytes() == pytest.approx(pc.info.num_cells * (48.0 + 4.0 * nd) + 16.0 * pc.info.ndofs)
            assert pp.alg_bytes() == pytest.approx(pp.info.num_cells * (48.0 * nd + 4.0 * nd) + 16.0 * pp.info.ndofs)
            assert pc.info.plan_items > 0 and pc.info.plan_patterns > 0 and 0.0 < pc.info.plan_fill <= 1.0
            assert pc.info.plan_reoriented == pp.info.plan_reoriented and (pc.info.plan_reoriented > 0) == (lz == 0)
            if pc.info.plan_lz == pp.info.plan_lz:   # the same plan (the forms choose their own lz when left to)
                slots = pc.info.plan_items * pc.info.plan_lz * bx * by
                assert pp.info.device_bytes - pc.info.device_bytes == 48 * slots * (nd - 1) - 8 * (n * n + n)
            if lz == 1:
                assert pc.info.plan_lz == pp.info.plan_lz == 1
                assert pc.info.device_bytes < 2.0 * pp.info.device_bytes / nd


# ---- 7. refusals ----
def refused(status, *words, V, p, G=None, **tuning):
    import wave_fenics_amd as w
    with pytest.raises(w.WavehipError) as e:
        w.StiffnessOperator(V, p, C0, G=G, structured=False, tuning=tuning)
    assert e.value.status == status, (e.value.status, str(e.value))
    for word in words:
        assert word in str(e.value), (word, str(e.value))


INVALID, UNSUPPORTED = -1, -2   # WF_ERR_INVALID, WF_ERR_UNSUPPORTED (include/wavehip.h)


@pytest.mark.parametrize("kind", ["perturbed", "one_vertex", "tiny"])
def test_refused_meshes(gpu, oracle, kind):
    """A mesh that does not qualify: the request names the cell; without the request the same mesh creates and passes
    parity."""
    from wave_fenics_amd import mesh_io
    mesh, cell, _ = h.refusal_mesh(kind)
    p = 2
    V = mesh_io.create_functionspace(mesh, p)
    word = "clamp" if kind == "tiny" else "affine"
    refused(INVALID, f"cell {cell} ", word, V=V, p=p, geometry="per_cell")
    ref = h.reference_of(mesh, V, p)
    for tuning in ({}, {"geometry": "per_point"}, {"kernel": "march"}):
        op = stiffness(V, p, **tuning)
        assert op.kernel in ("march_idx", "batch_unique") and op.geometry == "per_point"
        assert np.abs(run(op, ref, gpu) - ref.yref).max() <= TOL_ORACLE * ref.scale
    if kind == "tiny":   # the clamp is the only obstacle
        from wave_fenics_amd._lib import WF_FLAG_NO_CLAMP
        assert stiffness(V, p, WF_FLAG_NO_CLAMP, geometry="per_cell").geometry == "per_cell"


def test_refused_requests(gpu, oracle):
    p = 2
    V = h.space("unit-asis", p)
    refused(UNSUPPORTED, "degree", V=h.space("unit-asis", 5), p=5, geometry="per_cell")
    K = oracle.StiffnessOperator(h.oracle_mesh(h.affine_mesh("unit-asis"), V), p)
    refused(UNSUPPORTED, "h_G", V=V, p=p, G=K.G, geometry="per_cell")
    refused(INVALID, "kernel", V=V, p=p, geometry="per_cell", kernel="batch")
    refused(INVALID, "kernel", V=V, p=p, geometry="per_cell", kernel="elementwise")
    refused(UNSUPPORTED, "owner", V=V, p=p, geometry="per_cell", update="owner")
    refused(INVALID, "axes", "off-diagonal", V=h.space("sheared-asis", p), p=p, geometry="per_cell", metric="axes")
    # the same requests without the field are today's operators
    assert stiffness(h.space("unit-asis", 5), 5).geometry == "per_point"
    assert stiffness(V, p, kernel="batch").kernel == "batch_unique"


def test_ordered_flag_still_takes_no_tuning(gpu):
    import wave_fenics_amd as w
    from wave_fenics_amd._lib import WF_FLAG_ORDERED
    with pytest.raises(w.WavehipError) as e:
        stiffness(h.space("unit-asis", 2), 2, WF_FLAG_ORDERED, geometry="per_cell")
    assert e.value.status == INVALID and "WF_FLAG_ORDERED" in str(e.value)


# ---- 8. defaults unchanged ----
@pytest.mark.parametrize("p", [2, 4])
def test_defaults_unchanged(gpu, p):
    """Without the request an affine mesh keeps the per-point operator; the mass operators ignore the field."""
    import wave_fenics_amd as w
    V = h.space("glued_rotated", p)
    nd = (p + 1) ** 3
    for tuning in (None, {"geometry": "per_point"}, {"geometry": "auto"}):
        op = w.StiffnessOperator(V, p, C0, structured=False, tuning=tuning)
        assert (op.kernel, op.geometry, op.metric, op.update) == ("march_idx", "per_point", "none", "none")
        assert op.info.plan_reoriented == 36
        assert op.alg_bytes() == pytest.approx(op.info.num_cells * (48.0 * nd + 4.0 * nd) + 16.0 * op.info.ndofs)
    a = w.MassOperatorLumped(V, p, structured=False)
    b = w.MassOperatorLumped(V, p, structured=False, tuning={"geometry": "per_cell"})
    assert (a.kernel, a.geometry, a.info.device_bytes) == (b.kernel, b.geometry, b.info.device_bytes)


# ---- 9. the loop ----
def mesh_file_case(oracle, tmp_path, p=3, n=(4, 3, 3), hi=(0.01, 0.0075, 0.0075)):
    """An unperturbed box written with cells and vertices renumbered at random (the route of
    test_mesh_io.test_rk4_from_mesh_file), the oracle's loop on the original box and the dof matching by coordinates."""
    from test_mesh_io import shuffled_box
    from wave_fenics_amd import mesh_io
    om, mesh, tags = shuffled_box(oracle, n, p, hi, 0.0)
    path = str(tmp_path / "mesh.xdmf")
    mesh_io.write_mesh(path, "planar3d", mesh, "planar3d_boundaries", tags)
    dt, spp = oracle.cfl_time_step(om, p, 1500.0, 0.5e6, CFL=0.25)
    ref = oracle.LinearGLLOpt(om, p, 1500.0, 0.5e6, 6e4)
    ref.init()
    ref.rk4(0.0, 5 * dt - 1e-13, dt)
    m2, t2 = mesh_io.read_mesh(path, "planar3d", "planar3d_boundaries")
    V = mesh_io.create_functionspace(m2, p)
    X = oracle.dof_coordinates(om)
    e = np.linalg.norm(om.x[om.geom_dofmap[:, 1]] - om.x[om.geom_dofmap[:, 0]], axis=1).min()
    qa = np.round(X / (1e-9 * e)).astype(np.int64)
    qb = np.round(V.dof_coordinates / (1e-9 * e)).astype(np.int64)
    ia, ib = np.lexsort(qa.T[::-1]), np.lexsort(qb.T[::-1])
    assert np.array_equal(qa[ia], qb[ib])
    return path, om, ref, V, t2, dt, ia, ib


def test_rk4_from_mesh_file_per_cell(gpu, oracle, tmp_path):
    from wave_fenics_amd import mesh_io
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    p = 3
    path, om, ref, V, t2, dt, ia, ib = mesh_file_case(oracle, tmp_path, p)
    assert mesh_io.cfl_time_step(V.mesh, p, 1500.0, 0.5e6, CFL=0.25)[0] == dt
    eqn = LinearGLLOpt(V, p, 1500.0, 0.5e6, 6e4, boundary=mesh_io.boundary_sets(V, t2), device=gpu, structured=False,
                       tuning={"geometry": "per_cell"})
    assert (eqn.stiff_op.kernel, eqn.stiff_op.geometry, eqn.stiff_op.metric) == ("march_idx", "per_cell", "axes")
    eqn.init()
    eqn.rk4_fused(0.0, 5 * dt - 1e-13, dt)
    u, v = eqn.u_n.cpu().numpy(), eqn.v_n.cpu().numpy()
    assert np.abs(u[ib] - ref.u_n[ia]).max() <= 1e-9 * np.abs(ref.u_n).max()
    assert np.abs(v[ib] - ref.v_n[ia]).max() <= 1e-9 * np.abs(ref.v_n).max()


def test_planar3d_geometry_option(gpu, oracle, tmp_path):
    """examples/planar3d --mesh FILE --geometry per_cell (the C++ wrappers' wf_tuning pass-through): the per-cell
    kernel is reported and the fields match the oracle; --geometry auto prints what no option prints."""
    p = 3
    path, om, ref, V, t2, dt, ia, ib = mesh_file_case(oracle, tmp_path, p)
    out = str(tmp_path / "bin")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), f"OUT={out}", f"{out}/planar3d"])
    outputs = {}
    for geometry in (None, "auto", "per_cell", "per_point"):
        dump = str(tmp_path / "uv.bin")
        extra = ["--geometry", geometry] if geometry else []
        r = subprocess.run([os.path.join(out, "planar3d"), "--mesh", path, "--degree", str(p), "--cfl", "0.25", "--steps", "5",
                            "--dump", dump] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Steps taken: 5" in r.stdout and f"Degrees of freedom: {om.ndofs}" in r.stdout
        outputs[geometry] = [ln for ln in r.stdout.splitlines() if "time" not in ln.lower() and "dof/s" not in ln.lower()]
        uv = np.fromfile(dump, dtype=np.float64)
        u, v = uv[: om.ndofs], uv[om.ndofs:]
        assert np.abs(u[ib] - ref.u_n[ia]).max() <= 1e-9 * np.abs(ref.u_n).max()
        assert np.abs(v[ib] - ref.v_n[ia]).max() <= 1e-9 * np.abs(ref.v_n).max()
        assert ("Stiffness geometry: per_cell" in r.stdout) == (geometry == "per_cell"), r.stdout
    assert outputs[None] == outputs["auto"] == outputs["per_point"]
    r = subprocess.run([os.path.join(out, "planar3d"), "--mesh", path, "--degree", "5", "--steps", "1", "--geometry", "per_cell"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WF_GEOMETRY_PER_CELL" in r.stdout + r.stderr
