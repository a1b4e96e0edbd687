"""Domain decomposition of the box mesh and the ghost exchange.

Replaces demo/gpu_scatter_mpi/VectorUpdater.hpp:21-230 (GPU pack + CUDA-aware
MPI point-to-point over the IndexMap neighbourhood) and the
la::Vector::scatter_fwd / scatter_rev(add) calls of common/LinearGLL.hpp:164-176:
one process per GPU.  Two transports carry the same index lists:
  "native": wf_updater_* of the C ABI (csrc/updater.hip) -- a grouped ncclSend/ncclRecv
            per neighbour on an RCCL communicator created inside libwavehip, i.e.
            one message per xGMI link for the 2x2x2 partition; the default for
            device vectors;
  "torch" : ONE torch.distributed all_to_all_single per update (gloo on CPU tensors
            for the multi-process CPU tests, or nccl); pack/unpack are the libwavehip
            gather/scatter kernels either way.

Partition: Cartesian px x py x pz (the idea of decompose3d /
compute_cartesian_indices in demo/gpu_cg/mesh.hpp:37-63), rank = rz + pz*(ry + py*rx).
Ownership: a lattice point shared by several ranks belongs to the lowest one, so
a rank's ghosts are the lower planes (I = 0, J = 0, K = 0) of its local lattice
where a lower neighbour exists.  Local vectors use the local lattice numbering
(ghosts interleaved, not appended) because the structured kernels address the
lattice implicitly; the owned/ghost split is carried by the index lists."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from functools import partialmethod

import numpy as np

from ._lib import WF_PART_INTERFACE, WF_PART_INTERIOR, WF_UPDATER_DEFAULT, BoxPartitionInfo, UpdaterDesc, _ip, check, lib
from .box import BoxMesh, FunctionSpace, IndexMap, _int3, create_box, create_functionspace
from .comm import Comm
from .operators import _ptr, _stream, gather, scatter, scatter_set


def decompose3d(nproc: int):
    """Split nproc into px >= py >= pz, as balanced as possible
    (1 -> 1x1x1, 2 -> 2x1x1, 4 -> 2x2x1, 8 -> 2x2x2; cf. demo/gpu_cg/mesh.hpp:37-48): wf_decompose3d."""
    procs = (ctypes.c_int * 3)()
    check(lib().wf_decompose3d(int(nproc), procs))
    return tuple(procs)


def rank_coords(rank: int, procs):
    """demo/gpu_cg/mesh.hpp:52-63 compute_cartesian_indices (z fastest)."""
    px, py, pz = procs
    return rank // (py * pz), (rank // pz) % py, rank % pz


def coords_rank(c, procs):
    px, py, pz = procs
    return c[2] + pz * (c[1] + py * c[0])


@dataclass
class GhostLists:
    """wavehip::GhostLists: the flat index lists as wf_box_partition fills them and wf_updater_desc takes them."""
    # Neighbour ranks ascending, one segment per neighbour; int32 local lattice indices.
    ndofs: int
    send_neighbors: np.ndarray      # intc
    send_offsets: np.ndarray        # int32, [len(send_neighbors) + 1], first entry 0
    send_indices: np.ndarray        # segment i: the owned dofs send_neighbors[i] holds as ghosts
    recv_neighbors: np.ndarray
    recv_offsets: np.ndarray
    ghost_positions: np.ndarray     # segment i: the ghosts recv_neighbors[i] owns, in the order it sends them


def _segments(nb, off, idx) -> dict:
    return {int(r): idx[off[i]:off[i + 1]] for i, r in enumerate(nb)}


@dataclass
class BoxPartition:
    procs: tuple
    rank: int
    coords: tuple
    n_local: tuple              # cells per direction on this rank
    degree: int
    mesh: BoxMesh
    V: FunctionSpace
    size_global: int            # global number of (owned) dofs
    owned_lo: tuple             # first owned lattice index per axis (0 or 1)
    ghosts: GhostLists          # the neighbour lists
    periodic: tuple = (False, False, False)        # axes whose upper face is identified with the lower one
    num_owned: int = 0
    face_tag: tuple = (0,) * 6                     # cfg1 tag of local face 2*axis + side, 0 = none (boundary_tags)

    # the lists keyed by neighbour rank (ascending): the owned dofs the neighbour holds as ghosts / my ghosts it owns
    send_fwd = property(lambda self: _segments(self.ghosts.send_neighbors, self.ghosts.send_offsets, self.ghosts.send_indices))
    recv_fwd = property(lambda self: _segments(self.ghosts.recv_neighbors, self.ghosts.recv_offsets, self.ghosts.ghost_positions))

    def owned_mask(self) -> np.ndarray:
        NX, NY, NZ = self.V.lattice
        m = np.ones((NZ, NY, NX), dtype=bool)
        if self.owned_lo[0]:
            m[:, :, 0] = False
        if self.owned_lo[1]:
            m[:, 0, :] = False
        if self.owned_lo[2]:
            m[0, :, :] = False
        return m.reshape(-1)


def create_distributed_box(n, degree: int, nproc: int, rank: int, lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0),
                           perturb: float = 0.0, seed: int = 42, build_dofmap: bool = False,
                           periodic=(False, False, False)) -> BoxPartition:
    """Weak-scaled box: n (int or 3-tuple) cells per direction PER RANK; the
    global mesh has (px*nx, py*ny, pz*nz) cells on [lo, hi].
    periodic[a] identifies the upper face of axis a with the lower one: the lower
    plane of EVERY rank is then a ghost plane and the neighbour relation wraps
    around, so a rank can be its own neighbour (with one rank per axis the exchange
    is a send/recv to self -- used to run the RCCL path on a single GPU).
    The partition, the ownership and the index lists are wf_box_partition's."""
    if np.isscalar(n):
        n = (int(n),) * 3
    periodic = tuple(bool(v) for v in periodic)
    info = BoxPartitionInfo()
    head = (_int3(n), int(degree), int(nproc), int(rank), (ctypes.c_int * 3)(*periodic), ctypes.byref(info))
    check(lib().wf_box_partition(*head, *[None] * 6))
    snb, rnb = np.zeros(7, dtype=np.intc), np.zeros(7, dtype=np.intc)
    soff, roff = np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32)
    sidx, ridx = np.empty(info.num_send_indices, dtype=np.int32), np.empty(info.num_recv_indices, dtype=np.int32)
    nbp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    check(lib().wf_box_partition(*head, nbp(snb), _ip(soff), _ip(sidx), nbp(rnb), _ip(roff), _ip(ridx)))
    procs, c = tuple(info.procs), tuple(info.coords)
    gn = tuple(procs[a] * n[a] for a in range(3))
    # local mesh = the rank's slab of the global vertex lattice (global coordinates;
    # the perturbation is drawn on the global mesh so that ranks agree on shared vertices)
    h = [(hi[a] - lo[a]) / gn[a] for a in range(3)]
    llo = tuple(lo[a] + h[a] * n[a] * c[a] for a in range(3))
    lhi = tuple(lo[a] + h[a] * n[a] * (c[a] + 1) for a in range(3))
    mesh = create_box(n, llo, lhi)
    if perturb > 0.0:
        gmesh_x = create_box(gn, lo, hi, perturb, seed).x.reshape(gn[2] + 1, gn[1] + 1, gn[0] + 1, 3)
        sl = tuple(slice(c[a] * n[a], (c[a] + 1) * n[a] + 1) for a in range(3))
        mesh.x = np.ascontiguousarray(gmesh_x[sl[2], sl[1], sl[0]].reshape(-1, 3))
    V = create_functionspace(mesh, degree, build_dofmap=build_dofmap)
    V.index_map = IndexMap(V.ndofs, 0, info.size_global)   # whole local lattice; see module docstring
    ns, nr = info.num_send_neighbors, info.num_recv_neighbors
    ghosts = GhostLists(V.ndofs, snb[:ns], soff[:ns + 1], sidx, rnb[:nr], roff[:nr + 1], ridx)
    return BoxPartition(procs, rank, c, tuple(n), degree, mesh, V, size_global=info.size_global,
                        owned_lo=tuple(info.owned_lo), ghosts=ghosts, periodic=periodic,
                        num_owned=info.num_owned, face_tag=tuple(info.face_tag))


def boundary_tags(part: BoxPartition) -> dict:
    """Facet tags of the rank's local box faces under the cfg1 convention
    (SURVEY 8d): global face x = lo -> tag 1 (Gamma_1), every other global face
    -> tag 2 (Gamma_2); interfaces between ranks carry no tag.
    Key = local face 2*axis + side."""
    return {f: t for f, t in enumerate(part.face_tag) if t}


class HipKernels:
    """Pack/unpack through libwavehip (no fallback)."""

    @staticmethod
    def gather(idx, src, out):
        gather(idx.numel(), idx, src, out)

    @staticmethod
    def scatter_set(idx, src, out):
        scatter_set(idx.numel(), idx, src, out)

    @staticmethod
    def scatter_add(idx, src, out):
        scatter(idx.numel(), idx, src, out)


class _NativeExchange:
    """wf_updater_* and wf_op_apply_overlapped of the C ABI (csrc/updater.hip); owns the wf_updater handle."""

    def __init__(self, ghosts: GhostLists, device, active: bool, group, kernels, comm):
        if device.type != "cuda":
            raise RuntimeError("transport='native' exchanges device vectors (RCCL)")
        self.comm = Comm.from_torch_distributed(group) if (comm is None and active) else comm
        g, nbp = ghosts, lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        d = UpdaterDesc(g.ndofs, len(g.send_neighbors), nbp(g.send_neighbors), _ip(g.send_offsets), _ip(g.send_indices),
                        len(g.recv_neighbors), nbp(g.recv_neighbors), _ip(g.recv_offsets), _ip(g.ghost_positions),
                        WF_UPDATER_DEFAULT)
        self.handle = ctypes.c_void_p()
        check(lib().wf_updater_create(self.comm._h if self.comm is not None else None, ctypes.byref(d),
                                      ctypes.byref(self.handle)))

    def _call(self, fn: str, x):
        check(getattr(lib(), fn)(self.handle, _ptr(x), _stream(x)))

    fwd_begin = partialmethod(_call, "wf_updater_fwd_begin")
    fwd_end = partialmethod(_call, "wf_updater_fwd_end")
    rev_begin = partialmethod(_call, "wf_updater_rev_begin")
    rev_end = partialmethod(_call, "wf_updater_rev_end")

    def overlapped_apply(self, op, x, y):
        check(lib().wf_op_apply_overlapped(op._h, self.handle, _ptr(x), _ptr(y), _stream(x)))

    def close(self):
        if self.handle is not None and self.handle.value:
            lib().wf_updater_destroy(self.handle)
            self.handle = None


class _TorchExchange:
    """ONE torch.distributed all_to_all_single per update on `group`; pack/unpack through `kernels` (libwavehip's
    gather/scatter unless a test passes a double)."""

    def __init__(self, ghosts: GhostLists, device, active: bool, group, kernels, comm):
        import torch
        import torch.distributed as dist
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        if world == 1 and active:
            raise RuntimeError("a self-neighbour (periodic) exchange on one rank needs transport='native'")
        self.active, self.group = active, group     # active: read by overlapped_apply alone
        self.kernels = HipKernels if kernels is None else kernels
        # entries per rank of the group, 0 for a rank that is no neighbour
        self.send_sizes = np.bincount(ghosts.send_neighbors, np.diff(ghosts.send_offsets), world).astype(int).tolist()
        self.recv_sizes = np.bincount(ghosts.recv_neighbors, np.diff(ghosts.recv_offsets), world).astype(int).tolist()
        self.d_indices = torch.from_numpy(ghosts.send_indices).to(device)          # scatter_fwd_indices
        self.d_ghost_pos = torch.from_numpy(ghosts.ghost_positions).to(device)
        # zero-length exchanges (a rank with no ghosts / no upper neighbour) keep a valid allocation behind the view
        buffer = lambda n: torch.zeros(max(n, 1), dtype=torch.float64, device=device)[:n]
        self.d_send_buffer, self.d_recv_buffer = buffer(self.d_indices.numel()), buffer(self.d_ghost_pos.numel())
        # a transport that cannot read device memory (gloo) is staged through the host
        self.staged = dist.is_initialized() and dist.get_backend(group) == "gloo" and device.type == "cuda"
        if self.staged:
            self.h_send = torch.zeros(max(self.d_indices.numel(), self.d_ghost_pos.numel()), dtype=torch.float64).pin_memory()
            self.h_recv = torch.zeros_like(self.h_send).pin_memory()
        self._work = self._side = None  # pending exchange; stream of overlapped_apply, created on first use

    def _post(self, out, out_sizes, inp, in_sizes):
        import torch.distributed as dist
        if self.staged:
            import torch
            hs, hr = self.h_send[: inp.numel()], self.h_recv[: out.numel()]
            hs.copy_(inp)
            torch.cuda.current_stream().synchronize()
            dist.all_to_all_single(hr, hs, out_sizes, in_sizes, group=self.group)
            out.copy_(hr, non_blocking=True)
            return
        self._work = dist.all_to_all_single(out, inp, out_sizes, in_sizes, group=self.group, async_op=True)

    def _wait(self):
        if self._work is not None:
            self._work.wait()
            self._work = None

    def fwd_begin(self, x):
        self.kernels.gather(self.d_indices, x, self.d_send_buffer)                  # VectorUpdater.hpp:110-111
        self._post(self.d_recv_buffer, self.recv_sizes, self.d_send_buffer, self.send_sizes)

    def fwd_end(self, x):
        self._wait()
        self.kernels.scatter_set(self.d_ghost_pos, self.d_recv_buffer, x)           # VectorUpdater.hpp:139-142

    def rev_begin(self, x):
        self.kernels.gather(self.d_ghost_pos, x, self.d_recv_buffer)                # VectorUpdater.hpp:165-168
        self._post(self.d_send_buffer, self.send_sizes, self.d_recv_buffer, self.recv_sizes)

    def rev_end(self, x):
        self._wait()
        self.kernels.scatter_add(self.d_indices, self.d_send_buffer, x)             # VectorUpdater.hpp:196-198

    def overlapped_apply(self, op, x, y):
        import torch
        if not self.active:             # nothing to exchange, and perhaps no process group: the operator, unsplit
            return op(x, y)
        main = torch.cuda.current_stream(x.device)
        side = self._side = self._side or torch.cuda.Stream(device=x.device)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            self.fwd_begin(x)
            self.fwd_end(x)
            op.apply_part(x, y, WF_PART_INTERFACE)
            self.rev_begin(y)
        op.apply_part(x, y, WF_PART_INTERIOR)
        # the reverse add lands on owned entries of y that the interior part may hold between its read and its write
        # (the owner-computes box kernel updates y with plain loads and stores), so it waits for the interior part
        side.wait_stream(main)
        with torch.cuda.stream(side):
            self.rev_end(y)
        main.wait_stream(side)

    def close(self):
        pass


class VectorUpdater:
    """VectorUpdater<T, Alloc> of demo/gpu_scatter_mpi/VectorUpdater.hpp:21-230.

    update_fwd(x): owners -> ghosts (VectorUpdater.hpp:148-152);
    update_rev(x): ghosts -> owners, accumulating (VectorUpdater.hpp:204-208).
    scatter_fwd / scatter_rev are the la::Vector spellings used by
    common/LinearGLL.hpp.  The _begin/_end split of the reference is kept:
    begin packs and posts the exchange, end waits and unpacks.

    transport "native" (default for device vectors unless the process group is gloo):
    wf_updater_* over an RCCL communicator (`comm`, created from torch.distributed's
    ranks when not given).  transport "torch": all_to_all_single on `group`."""

    def __init__(self, part: BoxPartition, device=None, group=None, kernels=None, transport: str | None = None,
                 comm=None):
        import torch
        import torch.distributed as dist
        self.part = part
        self.device = torch.device("cpu") if device is None else device
        backend = dist.get_backend(group) if dist.is_initialized() else None
        if transport is None:
            transport = "native" if (self.device.type == "cuda" and backend != "gloo" and kernels is None) else "torch"
        if transport not in ("native", "torch"):
            raise ValueError("transport must be 'native' or 'torch'")
        self.transport = transport
        g = part.ghosts
        self.send_neighbors, self.recv_neighbors = g.send_neighbors.tolist(), g.recv_neighbors.tolist()
        self.h_indices, self.h_ghost_pos = g.send_indices, g.ghost_positions
        self.active = bool(self.send_neighbors or self.recv_neighbors)
        make = _NativeExchange if transport == "native" else _TorchExchange
        self._exchange = make(g, self.device, self.active, group, kernels, comm)

    # native transport only: its RCCL communicator and its wf_updater handle (None once closed)
    comm = property(lambda self: self._exchange.comm)
    _h = property(lambda self: self._exchange.handle)

    def close(self):
        self._exchange.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _step(self, name: str, x):
        if self.active:
            getattr(self._exchange, name)(x)

    # -- forward: owners -> ghosts --------------------------------------------
    update_fwd_begin = partialmethod(_step, "fwd_begin")
    update_fwd_end = partialmethod(_step, "fwd_end")

    def update_fwd(self, x):
        self.update_fwd_begin(x)
        self.update_fwd_end(x)

    # -- reverse: ghosts -> owners (add) ---------------------------------------
    update_rev_begin = partialmethod(_step, "rev_begin")
    update_rev_end = partialmethod(_step, "rev_end")

    def update_rev(self, x):
        self.update_rev_begin(x)
        self.update_rev_end(x)

    scatter_fwd = update_fwd
    scatter_rev = update_rev


def overlapped_apply(op, updater: VectorUpdater, x, y):
    """y += A x on a domain-decomposed mesh with BOTH halo directions hidden
    (LinearGLL.hpp:164-176 = scatter_fwd(x); apply; scatter_rev(y)):

        halo chain : update_fwd(x) -> apply(INTERFACE) -> update_rev(y)
        beside it  : apply(INTERIOR)                       (reads no ghost value)

    The interior part is one launch (splitting it further costs whole rounds of
    workgroups: 3 launches took 0.36 ms against 0.26 ms for the unsplit operator at
    cfg2), the interface cells and the two exchanges run beside it on a second HIP
    stream and fill its tail.  Requires op.set_ghost_faces(...) == True.
    Native transport: the whole sequence is wf_op_apply_overlapped of the C ABI."""
    if not x.is_cuda:
        raise RuntimeError("overlapped_apply needs device vectors")
    updater._exchange.overlapped_apply(op, x, y)


def owned_boundary_set(updater: VectorUpdater, V, idx, m, device):
    """A boundary dof set of a domain-decomposed mesh (indices, rank-local collocated facet masses)
    reduced to OWNED dofs with fully assembled masses: the rank-local masses are accumulated to
    their owners once at setup (scatter_rev), so that the boundary term b[i] += s m[i] v[i] is
    applied by the owner alone and needs no ghost value of v -- the second forward update per
    stage of the reference (LinearGLL.hpp:167) disappears."""
    import torch
    idx = np.asarray(idx)
    dense = torch.zeros(V.ndofs, dtype=torch.float64, device=device)
    if idx.size:
        dense[torch.from_numpy(idx.astype(np.int64)).to(device)] = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float64)).to(device)
    updater.scatter_rev(dense)
    h = dense.cpu().numpy()
    sel = np.nonzero((h != 0.0) & updater.part.owned_mask())[0].astype(np.int32)
    return sel, h[sel]


def owned_boundary(updater: VectorUpdater, V, tags, tag: int, device):
    """owned_boundary_set for the faces of a box partition carrying `tag`."""
    from .linear_gll import facet_lumped_mass
    idx, m = facet_lumped_mass(V, tags, tag)
    return owned_boundary_set(updater, V, idx, m, device)
