"""The box host layer (csrc/box_space.cpp: wf_box_mesh, wf_box_dofmap, wf_box_facet_mass, wf_decompose3d,
wf_box_partition) through its Python wrappers, against the contract written with plain numpy in tests/box_helpers.py.
No GPU.  (Vertices and dofmaps against the oracle: test_abi.py::test_box_mesh_matches_oracle; the C++ wrappers against
the Python ones: test_cxx_partition_matches_python, test_product_facet_masses_vs_independent.)"""
import ctypes

import numpy as np
import pytest

import box_helpers as bh
from support import bits, wpackage as wlib  # noqa: F401

TAGS = {0: 1, 1: 2, 2: 2, 3: 2, 4: 2, 5: 2}


# ---------------------------------------------------------------------------------------------------------------------
# partition
# ---------------------------------------------------------------------------------------------------------------------
PARTITION_CASES = [
    # test_cxx_partition_matches_python
    (1, (2, 2, 2), 2, (1, 0, 0)), (1, (2, 1, 2), 3, (1, 1, 1)), (2, (2, 2, 1), 2, (1, 1, 0)), (4, (1, 2, 2), 2, (0, 0, 0)),
    (8, (1, 2, 1), 2, (0, 0, 0)), (8, (1, 1, 1), 3, (1, 0, 1)), (6, (2, 1, 1), 1, (0, 1, 0)),
    # test_periodic_partition_lists
    (4, (1, 2, 2), 2, (1, 1, 1)), (8, (1, 1, 1), 2, (1, 0, 1)), (2, (2, 2, 2), 1, (0, 1, 0)),
    # one rank, no periodic axis: empty lists
    (1, (2, 3, 1), 2, (0, 0, 0)),
    # (7, 1, 1) and (3, 2, 2)
    (7, (1, 2, 1), 2, (0, 0, 0)), (7, (2, 1, 1), 1, (1, 0, 0)), (12, (1, 1, 2), 2, (0, 0, 0)), (12, (1, 1, 1), 1, (1, 1, 1)),
    # a periodic axis with exactly two ranks: the upper and the lower neighbour are one rank, two segments reach it
    (2, (2, 1, 2), 3, (1, 0, 0)), (4, (1, 2, 1), 2, (1, 1, 0)),
    # one cell at P1
    (1, (1, 1, 1), 1, (0, 0, 0)), (1, (1, 1, 1), 1, (1, 1, 1)), (8, (1, 1, 1), 1, (0, 0, 0)), (2, (1, 1, 1), 1, (1, 0, 0)),
]


@pytest.mark.parametrize("world,n,p,per", PARTITION_CASES)
def test_partition_matches_restatement(wlib, world, n, p, per):
    from wave_fenics_amd.distributed import boundary_tags, create_distributed_box
    for rank in range(world):
        part = create_distributed_box(n, p, world, rank, periodic=per)
        ref = bh.partition(n, p, world, rank, per)
        assert tuple(part.procs) == ref["procs"] and tuple(part.coords) == ref["coords"]
        assert tuple(part.owned_lo) == ref["owned_lo"] and tuple(part.V.lattice) == ref["lattice"]
        assert part.size_global == ref["size_global"] and part.num_owned == ref["num_owned"]
        assert part.V.index_map.size_global == ref["size_global"] and part.V.ndofs == int(np.prod(ref["lattice"]))
        for got, want in ((part.send_fwd, ref["send"]), (part.recv_fwd, ref["recv"])):
            assert list(got) == sorted(want)                       # neighbours ascending
            for nb in want:
                assert got[nb].dtype == np.int32 and np.array_equal(got[nb], want[nb])
        assert boundary_tags(part) == ref["tags"]


def test_partition_shapes(wlib):
    """the named shapes of the cases above are what they are meant to be"""
    from wave_fenics_amd.distributed import create_distributed_box, decompose3d
    assert decompose3d(7) == (7, 1, 1) and decompose3d(12) == (3, 2, 2) and decompose3d(1) == (1, 1, 1)
    one = create_distributed_box((2, 3, 1), 2, 1, 0)
    assert one.send_fwd == {} and one.recv_fwd == {} and one.num_owned == one.V.ndofs == one.size_global
    # two ranks on a periodic x axis: the upper and the (wrapped) lower neighbour of rank 0 are both rank 1, which so
    # appears in the send and in the receive list, with the whole upper / lower x plane
    part = create_distributed_box((2, 1, 2), 3, 2, 0, periodic=(1, 0, 0))
    NX, NY, NZ = part.V.lattice
    assert list(part.send_fwd) == [1] and list(part.recv_fwd) == [1]
    assert np.array_equal(part.send_fwd[1], NX - 1 + NX * np.arange(NY * NZ))
    assert np.array_equal(part.recv_fwd[1], NX * np.arange(NY * NZ))
    # with y periodic on one rank as well, directions (1, 0, 0) and (1, 1, 0) both reach rank 1: two segments, the plane
    # over the owned y range and then the edge, and (0, 1, 0) reaches the rank itself
    part = create_distributed_box((2, 2, 1), 2, 2, 0, periodic=(1, 1, 0))
    NX, NY, NZ = part.V.lattice
    assert part.procs == (2, 1, 1) and list(part.send_fwd) == [0, 1] and part.owned_lo == (1, 1, 0)
    plane = np.array([NX - 1 + NX * (J + NY * K) for K in range(NZ) for J in range(1, NY)])
    edge = np.array([NX - 1 + NX * (NY - 1 + NY * K) for K in range(NZ)])
    assert np.array_equal(part.send_fwd[1], np.concatenate([plane, edge]))
    # four ranks, two on each periodic axis: every neighbour is reached by one direction
    part = create_distributed_box((1, 2, 1), 2, 4, 0, periodic=(1, 1, 0))
    NX, NY, NZ = part.V.lattice
    assert part.procs == (2, 2, 1) and list(part.send_fwd) == [1, 2, 3]
    assert part.send_fwd[3].size == NZ and part.send_fwd[2].size == (NY - 1) * NZ


# ---------------------------------------------------------------------------------------------------------------------
# facet masses
# ---------------------------------------------------------------------------------------------------------------------
# one box per degree: perturbed and not, one cell thick and not, unit and not
FACET_BOXES = [(1, (3, 2, 4), 0.2, (1.0, 1.0, 1.0)), (2, (3, 2, 4), 0.0, (1.0, 1.0, 1.0)), (3, (2, 3, 2), 0.25, (1.0, 2.0, 0.5)),
               (4, (2, 2, 2), 0.15, (0.01, 0.01, 0.02)), (5, (1, 2, 3), 0.2, (1.0, 1.0, 1.0)), (6, (2, 1, 2), 0.0, (2.0, 1.0, 1.0)),
               (7, (2, 2, 1), 0.2, (1.0, 1.0, 1.0))]


def _box(w, p, n, perturb, hi):
    mesh = w.create_box(n, hi=hi, perturb=perturb)
    V = w.create_functionspace(mesh, p)
    weight = 0.25 + np.random.default_rng(5).uniform(0.0, 2.0, mesh.ncells)
    return mesh, V, weight


def test_facet_mass_matches_restatement(wlib):
    """linear_gll.facet_lumped_mass (the library's loop) against the numpy form: index sets identical, masses to 1e-14
    relative, the project's facet-mass tolerance"""
    from wave_fenics_amd.linear_gll import facet_lumped_mass
    worst, count = 0.0, 0
    for p, n, perturb, hi in FACET_BOXES:
        mesh, V, weight = _box(wlib, p, n, perturb, hi)
        pts, wts, _ = wlib.tabulate_gll(p)
        for cw in (None, weight):
            for tag in (1, 2):
                idx, m = facet_lumped_mass(V, TAGS, tag, cw)
                ri, rm = bh.facet_lumped_mass(V, pts, wts, TAGS, tag, cw)
                assert idx.dtype == np.int32 and np.array_equal(idx, ri)
                err = np.abs(m / rm - 1.0).max()
                worst, count = max(worst, err), count + idx.size
                assert err <= 1e-14, (p, n, tag, cw is not None, err)
    print(f"FACET MASS library vs numpy: {count} masses, worst relative difference {worst:.3e}")


def test_facet_mass_tags(wlib):
    """any tag value and any subset of faces; faces without the tag, and faces the dict does not name, give nothing"""
    from wave_fenics_amd.linear_gll import facet_lumped_mass
    mesh, V, weight = _box(wlib, 2, (3, 2, 2), 0.2, (1.0, 1.0, 1.0))
    pts, wts, _ = wlib.tabulate_gll(2)
    for tags, tag in (({3: 7, 4: 7, 0: 2}, 7), ({5: 1}, 1), ({0: 1, 1: 1}, 2), ({}, 1)):
        idx, m = facet_lumped_mass(V, tags, tag, weight)
        ri, rm = bh.facet_lumped_mass(V, pts, wts, tags, tag, weight)
        assert np.array_equal(idx, ri) and (idx.size == 0 or np.abs(m / rm - 1.0).max() <= 1e-14)
    with pytest.raises(ValueError):
        facet_lumped_mass(V, TAGS, 1, np.ones(mesh.ncells + 1))
    # no dofmap is needed (the benchmark's partition has none)
    V0 = wlib.create_functionspace(mesh, 2, build_dofmap=False)
    assert V0.dofmap.shape == (0, 27)
    a, b = facet_lumped_mass(V, TAGS, 2, weight), facet_lumped_mass(V0, TAGS, 2, weight)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def test_box_and_file_path_agree_bitwise(wlib):
    """one loop behind both: the box path equals mesh_io.facet_lumped_mass on the same space with the same facets listed
    as (cell, axis, side), bit for bit"""
    from wave_fenics_amd import linear_gll, mesh_io
    for p, n, perturb, hi in FACET_BOXES:
        mesh, V, weight = _box(wlib, p, n, perturb, hi)
        cells = np.arange(mesh.ncells).reshape(n[2], n[1], n[0])
        of_face = {0: cells[:, :, 0], 1: cells[:, :, -1], 2: cells[:, 0, :], 3: cells[:, -1, :], 4: cells[0], 5: cells[-1]}
        for cw in (None, weight):
            for tag in (1, 2):
                facets = [(int(c), f // 2, f % 2) for f in range(6) if TAGS[f] == tag for c in of_face[f].reshape(-1)]
                bi, bm = linear_gll.facet_lumped_mass(V, TAGS, tag, cw)
                fi, fm = mesh_io.facet_lumped_mass(V, facets, cw)
                assert np.array_equal(bi, fi) and np.array_equal(bits(bm), bits(fm)), (p, n, tag)


# ---------------------------------------------------------------------------------------------------------------------
# time step, bad arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_one_cfl_function(wlib):
    from wave_fenics_amd import linear_gll, mesh_io
    assert linear_gll.cfl_time_step is mesh_io.cfl_time_step
    mesh = wlib.create_box((4, 3, 5), hi=(0.01, 0.01, 0.02), perturb=0.15)
    assert linear_gll.cfl_time_step(mesh, 3, 1500.0, 0.5e6, 0.25) == mesh_io.cfl_time_step(mesh, 3, 1500.0, 0.5e6, 0.25)


def test_bad_arguments(wlib):
    """an error code and a wf_last_error text, no crash"""
    from wave_fenics_amd import _lib
    L = wlib.lib()
    i3 = lambda *v: (ctypes.c_int * 3)(*v)
    info = _lib.BoxPartitionInfo()
    none6 = [None] * 6

    def refused(rc, *words):
        msg = L.wf_last_error().decode()
        assert rc == -1 and all(word in msg for word in words), (rc, msg)

    n, per = i3(2, 2, 2), i3(0, 0, 0)
    assert L.wf_box_partition(n, 2, 4, 3, per, ctypes.byref(info), *none6) == 0
    refused(L.wf_box_partition(n, 2, 4, 4, per, ctypes.byref(info), *none6), "wf_box_partition", "rank")
    refused(L.wf_box_partition(n, 2, 4, -1, per, ctypes.byref(info), *none6), "wf_box_partition", "rank")
    refused(L.wf_box_partition(i3(2, 0, 2), 2, 4, 0, per, ctypes.byref(info), *none6), "wf_box_partition", "n must")
    for degree in (0, 9):
        refused(L.wf_box_partition(n, degree, 4, 0, per, ctypes.byref(info), *none6), "wf_box_partition", "degree")
    refused(L.wf_box_partition(n, 2, 4, 0, per, None, *none6), "wf_box_partition", "info")
    nb = (ctypes.c_int * 7)()
    refused(L.wf_box_partition(n, 2, 4, 0, per, ctypes.byref(info), nb, None, None, None, None, None), "all six")
    x, gd = np.zeros((27, 3)), np.zeros((8, 8), dtype=np.int32)
    d3 = lambda *v: (ctypes.c_double * 3)(*v)
    refused(L.wf_box_mesh(i3(2, 2, 0), d3(0, 0, 0), d3(1, 1, 1), _lib._dp(x), _lib._ip(gd)), "wf_box_mesh", "n must")
    dm = np.zeros((8, 27), dtype=np.int32)
    refused(L.wf_box_dofmap(2, i3(0, 2, 2), _lib._ip(dm)), "wf_box_dofmap", "n must")
    for degree in (0, 9):
        refused(L.wf_box_dofmap(degree, n, _lib._ip(dm)), "wf_box_dofmap", "degree")
    tags, nout = (ctypes.c_int * 6)(1, 2, 2, 2, 2, 2), ctypes.c_int64(0)
    assert L.wf_box_mesh(n, d3(0, 0, 0), d3(1, 1, 1), _lib._dp(x), _lib._ip(gd)) == 0
    assert L.wf_box_facet_mass(2, n, _lib._dp(x), tags, 1, None, ctypes.byref(nout), None, None) == 0 and nout.value == 25
    refused(L.wf_box_facet_mass(2, n, _lib._dp(x), tags, 0, None, ctypes.byref(nout), None, None), "wf_box_facet_mass", "tag 0")
    refused(L.wf_box_facet_mass(2, i3(2, 2, 0), _lib._dp(x), tags, 1, None, ctypes.byref(nout), None, None), "n must")
    for degree in (0, 9):
        refused(L.wf_box_facet_mass(degree, n, _lib._dp(x), tags, 1, None, ctypes.byref(nout), None, None), "degree")
    refused(L.wf_decompose3d(0, i3(0, 0, 0)), "wf_decompose3d")
    with pytest.raises(wlib.WavehipError):
        wlib.create_box((2, 0, 2))


def test_box_space_sanitized(tmp_path):
    """memory safety of the host code: box_space.cpp, function_space.cpp and tables.cpp built into a stand-alone program
    with AddressSanitizer and UndefinedBehaviorSanitizer (host code only; nothing of it is loaded into this process),
    walking the cases above with the size-only call followed by the fill call into arrays of exactly those sizes, and the
    box written out as a dofmap mesh (csrc/box_mesh.h) against wf_box_dofmap, wf_box_mesh and box_vertex"""
    import os
    import subprocess
    from wave_fenics_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "wave_fenics_amd", "csrc")
    exe = str(tmp_path / "box_space_walk")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *san, "-I", os.path.join(root, "include"),
                           "-I", csrc] + [os.path.join(csrc, s) for s in ("box_space.cpp", "function_space.cpp", "tables.cpp")]
                          + [os.path.join(root, "tests", "cxx", "box_space_walk.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr
