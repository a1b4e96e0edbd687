"""What every test family uses: the GPU and library fixtures, error measures and the small box helpers.

A plain module, imported like the *_helpers.py modules (`from support import ...`).  Fixtures travel by import: pytest
registers an imported fixture in the importing module, so `from support import gpu  # noqa: F401` gives that module a
module-scoped `gpu` of its own.  The module imports without a GPU and without torch; torch is imported inside the
functions that need it."""
import numpy as np
import pytest

LD = np.longdouble
assert np.finfo(LD).eps < 2.0 ** -60, "the reference needs a long double wider than float64"
EPS = 2.0 ** -52


def open_gpu():
    """Assert a GPU, load the library, make device 0 current; the device."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import wave_fenics_amd as w
    w.lib()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def gpu():
    return open_gpu()


def built_lib():
    """wave_fenics_amd._lib with the library built and loaded (no GPU needed)."""
    from wave_fenics_amd import build
    build.build()
    from wave_fenics_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def wlib():
    return built_lib()


@pytest.fixture(scope="module")
def wpackage(oracle):
    """The package over a built and loaded library, for host tests that use its Python layer; the oracle they compare
    with is built first.  A module that calls it `w` or `wlib` imports it under that name."""
    built_lib()
    import wave_fenics_amd
    return wave_fenics_amd


def relerr(a, b, scale=None):
    """max|a - b| over max|b|, or over `scale` when given."""
    s = float(np.abs(b).max()) if scale is None else scale
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(s, 1e-300))


def ratio(got, ref, mag, B):
    """worst |got - ref| / (eps mag); every entry must satisfy |got - ref| <= B eps mag (absolute: exact where mag is 0).
    Returns (worst, all within the bound, index of the first entry outside it; -1 for an empty array)."""
    err = np.abs(np.asarray(got, dtype=LD) - np.asarray(ref, dtype=LD))
    mag = np.asarray(mag, dtype=LD)
    ok = err <= B * LD(EPS) * mag
    pos = mag > 0
    worst = float(np.max(err[pos] / (LD(EPS) * mag[pos]))) if pos.any() else 0.0
    return worst, bool(ok.all()), int(np.argmin(ok)) if ok.size else -1


def bits(a):
    """The bit patterns of a float64 array, to compare for equality."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def dev(a, gpu, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return t if dtype is None else t.to(dtype)


def lattice_x(vx, vy, vz):
    """Vertex coordinates of the rectilinear box with the given axes, x fastest."""
    Z, Y, X = np.meshgrid(vz, vy, vx, indexing="ij")
    return np.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], axis=1).copy()


def cells_per_batch(p):
    """CB of the column-thread batch kernels (cells_per_batch, csrc/common.h)"""
    return 256 // (p + 1) ** 2


def owner_columns(n, p, bx, by):
    """Columns of the owner form on the box n: lattice lines in pieces of p bx x p by."""
    return -(-(p * n[0] + 1) // (p * bx)) * -(-(p * n[1] + 1) // (p * by))


@pytest.fixture(scope="module")
def comm(gpu):
    """A communicator of one rank over RCCL, closed at teardown."""
    from wave_fenics_amd.comm import Comm
    c = Comm.single()
    assert c.rccl_version() >= 20000
    yield c
    c.close()


def oracle_module():
    """oracle.wave_oracle, for cached helpers that cannot take the `oracle` fixture."""
    from oracle import wave_oracle
    return wave_oracle


def make(oracle, n, p, perturb=0.2):
    """(oracle mesh, mesh, FunctionSpace) of the perturbed box n, the two checked to agree."""
    import wave_fenics_amd as w
    om = oracle.create_box(n, p, perturb=perturb)
    mesh = w.create_box(n, perturb=perturb)
    V = w.create_functionspace(mesh, p)
    assert np.array_equal(V.dofmap, om.dofmap) and np.array_equal(mesh.x, om.x)
    return om, mesh, V
