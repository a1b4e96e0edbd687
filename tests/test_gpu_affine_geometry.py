"""Per-cell geometry of the box stiffness operator (wf_tuning.geometry, wf_op_info_t.geometry).

A box whose cells are all affine stores one G_c = J^-1 J^-T |det J| per cell and the marching kernel
forms G at a point as G_c w_i w_j w_k; any other box keeps the per-point geometry.  Every operator is
checked against the CPU oracle (1e-12 of max|y|) and against the same box with the
per-point geometry forced (1e-13: the two differ only in how G is rounded)."""
import numpy as np
import pytest

from owner_helpers import apply_from_zero as apply
from owner_helpers import spaces
from support import gpu, lattice_x, relerr  # noqa: F401

pytestmark = pytest.mark.gpu

TOL_ORACLE = 1e-12
TOL_POINT = 1e-13


def check_box(oracle, gpu, p, om, V, expect, seed=0):
    import wave_fenics_amd as w
    x = np.random.default_rng(seed).uniform(-1, 1, om.ndofs)
    yref = np.zeros(om.ndofs)
    oracle.StiffnessOperator(om, p)(x, yref)
    op = w.StiffnessOperator(V, p, {"c0": 1500.0}, structured=True)
    pp = w.StiffnessOperator(V, p, {"c0": 1500.0}, structured=True, tuning={"geometry": "per_point"})
    assert op.kernel == "march_box" and pp.kernel == "march_box"
    assert op.geometry == expect and pp.geometry == "per_point"
    y, ypp = apply(op, x, gpu), apply(pp, x, gpu)
    assert relerr(y, yref) <= TOL_ORACLE, (p, expect, relerr(y, yref))
    assert relerr(y, ypp) <= TOL_POINT, (p, expect, relerr(y, ypp))
    return op, pp


AFFINE = ["unit", "anisotropic", "far", "graded", "sheared"]


@pytest.mark.parametrize("p,n", [(1, (6, 5, 4)), (2, (5, 4, 3)), (3, (4, 3, 3)), (4, (5, 3, 4))])
@pytest.mark.parametrize("case", AFFINE)
def test_affine_boxes_take_per_cell_geometry(gpu, oracle, p, n, case):
    if case == "unit":
        om, V = spaces(oracle, n, p)
    elif case == "anisotropic":
        om, V = spaces(oracle, n, p, hi=(2.0, 1.0, 0.5))
    elif case == "far":   # coordinates ~1, h ~ 0.1 / n: cfg2's coordinate-to-h ratio
        om, V = spaces(oracle, n, p, lo=(0.9,) * 3, hi=(1.0,) * 3)
    elif case == "graded":   # uneven spacing per axis, built with BoxMesh directly
        rng = np.random.default_rng(7)
        axes = [np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 2.0, m))]) for m in n]
        om, V = spaces(oracle, n, p, x=lattice_x(*axes))
    else:   # sheared parallelepiped, x += 0.25 y on a dyadic lattice: affinity is a bitwise test, and
        # x += 0.3 y on linspace coordinates rounds each vertex differently (that box takes per-point geometry)
        x = lattice_x(*[np.arange(m + 1) * 0.125 for m in n])
        x[:, 0] += 0.25 * x[:, 1]
        om, V = spaces(oracle, n, p, x=x)
    op, pp = check_box(oracle, gpu, p, om, V, "per_cell")
    # the geometry stream is gone: 48 B per cell instead of 48 B per point
    nd = (p + 1) ** 3
    assert op.info.device_bytes < 2.0 * pp.info.device_bytes / nd
    assert op.alg_bytes() == pytest.approx(op.info.num_cells * (48.0 + 4.0 * nd) + 16.0 * op.info.ndofs)


@pytest.mark.parametrize("p,n", [(2, (4, 4, 3)), (4, (4, 3, 3))])
@pytest.mark.parametrize("case", ["perturbed", "one_vertex"])
def test_non_affine_boxes_keep_per_point_geometry(gpu, oracle, p, n, case):
    if case == "perturbed":
        om, V = spaces(oracle, n, p, perturb=0.2)
    else:   # a uniform box with one interior vertex moved
        om, _ = spaces(oracle, n, p)
        x = om.x.copy()
        nx, ny, _ = n
        x[1 + (nx + 1) * (1 + (ny + 1) * 1), 1] += 0.01
        om, V = spaces(oracle, n, p, x=x)
    check_box(oracle, gpu, p, om, V, "per_point")


def test_per_cell_request_on_perturbed_box_fails(gpu, oracle):
    import wave_fenics_amd as w
    _, V = spaces(oracle, (3, 3, 3), 4, perturb=0.2)
    with pytest.raises(w.WavehipError):
        w.StiffnessOperator(V, 4, {"c0": 1500.0}, structured=True, tuning={"geometry": "per_cell"})
    _, V = spaces(oracle, (3, 3, 3), 4)
    op = w.StiffnessOperator(V, 4, {"c0": 1500.0}, structured=True, tuning={"geometry": "per_cell"})
    assert op.geometry == "per_cell"


@pytest.mark.parametrize("p,n,lz", [(4, (6, 5, 11), 3), (2, (8, 7, 9), 2)])
def test_parts_sum_to_the_full_apply(gpu, oracle, p, n, lz):
    import torch
    import wave_fenics_amd as w
    from wave_fenics_amd._lib import WF_PART_INTERFACE, WF_PART_INTERIOR, WF_PART_INTERIOR_A, WF_PART_INTERIOR_B
    _, V = spaces(oracle, n, p)
    K = w.StiffnessOperator(V, p, {"c0": 1500.0}, tuning={"lz": lz})
    assert K.geometry == "per_cell"
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, V.ndofs)).to(gpu)
    yfull = torch.zeros_like(x)
    K(x, yfull)
    assert K.set_ghost_faces(True, False, True)
    for parts in ((WF_PART_INTERIOR, WF_PART_INTERFACE), (WF_PART_INTERIOR_A, WF_PART_INTERFACE, WF_PART_INTERIOR_B)):
        y = torch.zeros_like(x)
        for part in parts:
            K.apply_part(x, y, part)
        torch.cuda.synchronize()
        assert relerr(y.cpu().numpy(), yfull.cpu().numpy()) <= TOL_POINT, parts


@pytest.mark.parametrize("p,n", [(2, (7, 6, 9)), (4, (6, 5, 7))])
def test_per_cell_applies_are_repeatable(gpu, oracle, p, n):
    import torch
    import wave_fenics_amd as w
    _, V = spaces(oracle, n, p, hi=(1.0, 0.7, 1.3))
    op = w.StiffnessOperator(V, p, structured=True)
    assert op.geometry == "per_cell"
    x = torch.rand(V.ndofs, dtype=torch.float64, device=gpu)
    ref, worst = None, 0.0
    for _ in range(100):
        y = torch.zeros_like(x)
        op(x, y)
        if ref is None:
            ref = y.clone()
        else:
            worst = max(worst, float((y - ref).abs().max() / ref.abs().max()))
    assert worst <= 1e-14, worst


def test_full_size_bench_input(gpu):
    """cfg2 (P4, 54^3 cells), the benchmark's input sin(2 pi X): per cell against per point.  The two
    differ by the rounding of G (the per-point J is a cancelling sum over the vertices)."""
    import torch
    import wave_fenics_amd as w
    p, n = 4, 54
    V = w.create_functionspace(w.create_box(n), p)
    pc = w.StiffnessOperator(V, p, {"c0": 1500.0})
    assert pc.geometry == "per_cell" and pc.kernel == "march_box"
    pts, _, _ = w.tabulate_gll(p)   # dof x coordinates, as bench.py builds them
    xs = np.concatenate([(np.arange(n)[:, None] + pts[None, :p]).reshape(-1), [float(n)]]) / n
    x = torch.sin(2 * np.pi * torch.from_numpy(xs).to(gpu)).repeat((p * n + 1) ** 2).contiguous()
    y = torch.zeros_like(x)
    pc(x, y)
    del pc
    pp = w.StiffnessOperator(V, p, {"c0": 1500.0}, tuning={"geometry": "per_point"})
    assert pp.geometry == "per_point"
    ypp = torch.zeros_like(x)
    pp(x, ypp)
    torch.cuda.synchronize()
    err = float((y - ypp).abs().max() / ypp.abs().max())
    print(f"P4 54^3 sin(2 pi X): per cell vs per point max|dy|/max|y| = {err:.3e}")
    assert err <= 1e-11
