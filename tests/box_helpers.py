"""The box host layer's contract, written out with plain numpy and loops: what wf_box_partition and wf_box_facet_mass
(csrc/box_space.cpp) must give, independent of the library.  These are the functions the Python package held itself
before the rules moved into the library; tests/test_box_host.py compares the library with them."""
import numpy as np


# ---------------------------------------------------------------------------------------------------------------------
# Cartesian partition: px >= py >= pz, rank z-fastest, the lowest rank owns a shared point, neighbours ascending,
# the directions to one neighbour concatenated in (dx, dy, dz) loop order
# ---------------------------------------------------------------------------------------------------------------------
def decompose3d(nproc):
    best = None
    for a in range(1, nproc + 1):
        if nproc % a:
            continue
        for b in range(1, nproc // a + 1):
            if (nproc // a) % b:
                continue
            c = nproc // a // b
            dims = tuple(sorted((a, b, c), reverse=True))
            score = (dims[0] - dims[2], dims[0])
            if best is None or score < best[0]:
                best = (score, dims)
    return best[1]


def _axis_range(kind, lo, hi):
    """kind -1: the lower plane (index 0); +1: the upper plane (index hi); 0: the owned range."""
    if kind < 0:
        return np.array([0])
    if kind > 0:
        return np.array([hi])
    return np.arange(lo, hi + 1)


def partition(n, p, nproc, rank, periodic=(False, False, False)):
    """dict of procs, coords, owned_lo, lattice, size_global, num_owned, send, recv (neighbour rank -> int32 local
    lattice indices) and tags (local face 2*axis + side -> cfg1 tag) of one rank's part; n cells per rank."""
    procs = decompose3d(nproc)
    px, py, pz = procs
    c = (rank // (py * pz), (rank // pz) % py, rank % pz)
    periodic = tuple(bool(v) for v in periodic)
    NX, NY, NZ = (p * n[a] + 1 for a in range(3))
    owned_lo = tuple(1 if (c[a] > 0 or periodic[a]) else 0 for a in range(3))
    hi_idx = (NX - 1, NY - 1, NZ - 1)
    send, recv = {}, {}

    def lattice_indices(kinds):
        ix = _axis_range(kinds[0], owned_lo[0], hi_idx[0])
        iy = _axis_range(kinds[1], owned_lo[1], hi_idx[1])
        iz = _axis_range(kinds[2], owned_lo[2], hi_idx[2])
        K, J, I = np.meshgrid(iz, iy, ix, indexing="ij")
        return (I + NX * (J + NY * K)).reshape(-1).astype(np.int32)

    def append(lists, nb, idx):
        lists[nb] = np.concatenate([lists[nb], idx]) if nb in lists else idx

    rank_of = lambda q: q[2] + pz * (q[1] + py * q[0])
    wrap = lambda q: tuple(q[a] % procs[a] if periodic[a] else q[a] for a in range(3))
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                d = (dx, dy, dz)
                if d == (0, 0, 0):
                    continue
                up = wrap(tuple(c[a] + d[a] for a in range(3)))          # holds my upper plane(s) as ghosts
                if all(0 <= up[a] < procs[a] for a in range(3)):
                    append(send, rank_of(up), lattice_indices(d))
                dn = wrap(tuple(c[a] - d[a] for a in range(3)))          # owns my lower plane(s)
                if all(0 <= dn[a] < procs[a] for a in range(3)):
                    append(recv, rank_of(dn), lattice_indices(tuple(-v for v in d)))
    tags = {}
    for axis in range(3):
        if periodic[axis]:
            continue
        if c[axis] == 0:
            tags[2 * axis] = 1 if axis == 0 else 2
        if c[axis] == procs[axis] - 1:
            tags[2 * axis + 1] = 2
    return dict(procs=procs, coords=c, owned_lo=owned_lo, lattice=(NX, NY, NZ),
                size_global=int(np.prod([p * procs[a] * n[a] + (0 if periodic[a] else 1) for a in range(3)])),
                num_owned=(NX - owned_lo[0]) * (NY - owned_lo[1]) * (NZ - owned_lo[2]), send=send, recv=recv, tags=tags)


# ---------------------------------------------------------------------------------------------------------------------
# collocated facet masses of the tagged box faces, vectorised over the facets of a face
# ---------------------------------------------------------------------------------------------------------------------
def facet_lumped_mass(V, pts, w, tag_of_face, tag, cell_weight=None):
    """m[i] = sum_facets w_a w_b |dx/ds x dx/dt| on the faces 2*axis + side carrying tag; pts, w: the GLL rule on
    [0, 1] with P + 1 points.  Returns (ascending dof indices int32, masses)."""
    mesh = V.mesh
    p = V.degree
    n = p + 1
    nx, ny, nz = mesh.n
    NX, NY, NZ = V.lattice
    cz, cy, cx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    cid = cx + nx * (cy + ny * cz)
    acc = np.zeros(NX * NY * NZ)
    touched = np.zeros(NX * NY * NZ, dtype=bool)
    for axis, (cc, nn_) in enumerate(((cx, nx), (cy, ny), (cz, nz))):
        for side in (0, 1):
            if tag_of_face.get(2 * axis + side) != tag:
                continue
            cells = cid[cc == (0 if side == 0 else nn_ - 1)].reshape(-1)
            ta, tb = [d for d in range(3) if d != axis]
            bb, aa = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
            aa, bb = aa.reshape(-1), bb.reshape(-1)
            X = np.zeros((n * n, 3))
            X[:, axis] = float(side)
            X[:, ta] = pts[aa]
            X[:, tb] = pts[bb]
            # Q1 derivative table, vertex v = a + 2b + 4c
            dphi = np.zeros((3, n * n, 8))
            for v in range(8):
                bits = (v & 1, (v >> 1) & 1, (v >> 2) & 1)
                f = [X[:, d] if bits[d] else 1.0 - X[:, d] for d in range(3)]
                g = [np.ones(n * n) if bits[d] else -np.ones(n * n) for d in range(3)]
                dphi[0, :, v] = g[0] * f[1] * f[2]
                dphi[1, :, v] = f[0] * g[1] * f[2]
                dphi[2, :, v] = f[0] * f[1] * g[2]
            xc = mesh.x[mesh.geom_dofmap[cells]]
            J = np.einsum("fvi,jqv->fqij", xc, dphi)
            nrm = np.linalg.norm(np.cross(J[:, :, :, ta], J[:, :, :, tb]), axis=2)
            wq = (w[aa] * w[bb])[None, :] * nrm
            if cell_weight is not None:
                wq = wq * np.asarray(cell_weight)[cells][:, None]
            loc = np.zeros((n * n, 3), dtype=np.int64)
            loc[:, axis] = side * p
            loc[:, ta] = aa
            loc[:, tb] = bb
            ccx, ccy, ccz = cells % nx, (cells // nx) % ny, cells // (nx * ny)
            I = p * ccx[:, None] + loc[None, :, 0]
            Jd = p * ccy[:, None] + loc[None, :, 1]
            K = p * ccz[:, None] + loc[None, :, 2]
            dofs = (I + NX * (Jd + NY * K)).reshape(-1)
            np.add.at(acc, dofs, wq.reshape(-1))
            touched[dofs] = True
    idx = np.nonzero(touched)[0].astype(np.int32)
    return idx, acc[idx]
