// wavehip_box.hpp -- host-side box mesh / function space in C++ (the arrays a
// dolfinx::mesh::create_box + fem::create_functionspace pair would provide,
// demo/gpu_operator/main.cpp:60-72), with this engine's lexicographic numbering,
// the collocated facet masses of the boundary form (demo/cpu_planar3d/forms.ufl:19-24)
// and the Cartesian partition of the box.
// Thin wrappers over the host-only C ABI (wf_box_*, wf_decompose3d; csrc/box_space.cpp),
// shared with the Python package (box.py, linear_gll.py, distributed.py).
#pragma once

#include <array>
#include <cstdint>
#include <map>
#include <vector>

#include "wavehip.hpp"

namespace wavehip {

struct BoxMesh {
  std::array<int, 3> n{};                    // cells per direction
  std::vector<double> x;                     // [nverts][3]
  std::vector<std::int32_t> geom_dofmap;     // [ncells][8], vertex v = a + 2b + 4c
  std::int32_t ncells() const { return n[0] * n[1] * n[2]; }
  std::int32_t nverts() const { return (n[0] + 1) * (n[1] + 1) * (n[2] + 1); }
};

/// mesh::create_box(comm, {lo, hi}, {nx, ny, nz}, hexahedron)
inline BoxMesh create_box(std::array<int, 3> n, std::array<double, 3> lo = {0, 0, 0},
                          std::array<double, 3> hi = {1, 1, 1})
{
  BoxMesh m;
  m.n = n;
  m.x.resize((std::size_t)m.nverts() * 3);
  m.geom_dofmap.resize((std::size_t)m.ncells() * 8);
  check(wf_box_mesh(n.data(), lo.data(), hi.data(), m.x.data(), m.geom_dofmap.data()));
  return m;
}

/// The data of fem::create_functionspace(mesh, Lagrange(hexahedron, degree, gll_warped)).
struct BoxSpace {
  const BoxMesh* mesh = nullptr;
  int degree = 0;
  std::array<int, 3> lattice{};              // (NX, NY, NZ)
  std::vector<std::int32_t> dofmap;          // [ncells][nd], tensor order (empty if !build_dofmap)
  std::int32_t ndofs() const { return lattice[0] * lattice[1] * lattice[2]; }

  Space space() const
  {
    Space S;
    S.degree = degree;
    S.ncells = mesh->ncells();
    S.ndofs = ndofs();
    S.dofmap = dofmap.data();
    S.nverts = mesh->nverts();
    S.x = mesh->x.data();
    S.geom_dofmap = mesh->geom_dofmap.data();
    return S;
  }
};

inline BoxSpace create_functionspace(const BoxMesh& mesh, int degree, bool build_dofmap = true)
{
  BoxSpace V;
  V.mesh = &mesh;
  V.degree = degree;
  for (int a = 0; a < 3; ++a) V.lattice[a] = degree * mesh.n[a] + 1;
  if (build_dofmap) {
    V.dofmap.resize((std::size_t)mesh.ncells() * (degree + 1) * (degree + 1) * (degree + 1));
    check(wf_box_dofmap(degree, mesh.n.data(), V.dofmap.data()));
  }
  return V;
}

/// Collocated facet mass of the box faces carrying `tag`: m[i] = sum w_q |J_facet|
/// (the diagonal GLL form of inner(g, v) * ds(tag), forms.ufl:19-24).
/// tag_of_face: local face 2*axis + side -> tag.  Returns (dof indices, masses).
inline std::pair<std::vector<std::int32_t>, std::vector<double>>
facet_lumped_mass(const BoxSpace& V, const std::map<int, int>& tag_of_face, int tag)
{
  int face_tag[6] = {0, 0, 0, 0, 0, 0};
  for (auto& kv : tag_of_face)
    if (kv.first >= 0 && kv.first < 6) face_tag[kv.first] = kv.second;
  std::int64_t nout = 0;
  check(wf_box_facet_mass(V.degree, V.mesh->n.data(), V.mesh->x.data(), face_tag, tag, nullptr, &nout, nullptr, nullptr));
  std::pair<std::vector<std::int32_t>, std::vector<double>> out;
  out.first.resize((std::size_t)nout);
  out.second.resize((std::size_t)nout);
  check(wf_box_facet_mass(V.degree, V.mesh->n.data(), V.mesh->x.data(), face_tag, tag, nullptr, &nout, out.first.data(),
                          out.second.data()));
  return out;
}

// ---- domain decomposition (idea of demo/gpu_cg/mesh.hpp:37-63) -------
/// Split nproc into px >= py >= pz, as balanced as possible (1, 2x1x1, 2x2x1, 2x2x2).
inline std::array<int, 3> decompose3d(int nproc)
{
  std::array<int, 3> procs{};
  check(wf_decompose3d(nproc, procs.data()));
  return procs;
}
/// rank = rz + pz*(ry + py*rx)  (compute_cartesian_indices, z fastest)
inline std::array<int, 3> rank_coords(int rank, const std::array<int, 3>& procs)
{
  return {rank / (procs[1] * procs[2]), (rank / procs[2]) % procs[1], rank % procs[2]};
}
inline int coords_rank(const std::array<int, 3>& c, const std::array<int, 3>& procs)
{
  return c[2] + procs[2] * (c[1] + procs[1] * c[0]);
}

/// One rank's part of a Cartesian partition of the box: local mesh and space, the
/// ghost lists for VectorUpdater, the owned/ghost split.  A lattice point shared by
/// several ranks belongs to the lowest one, so the ghosts of a rank are its lower
/// lattice planes; local vectors keep the lattice numbering (ghosts interleaved).
struct BoxPartition {
  std::array<int, 3> procs{1, 1, 1}, coords{0, 0, 0}, n_local{};
  std::array<bool, 3> periodic{false, false, false};
  std::array<int, 3> owned_lo{0, 0, 0};       // first owned lattice index per axis
  int rank = 0, degree = 0;
  std::int64_t size_global = 0, owned_count = 0;
  std::array<int, 6> face_tag{};              // cfg1 tag of local face 2*axis + side, 0 = none
  BoxMesh mesh;
  BoxSpace V;
  GhostLists ghosts;

  std::int64_t num_owned() const { return owned_count; }
  bool owned(std::int32_t dof) const
  {
    const int I = dof % V.lattice[0], J = (dof / V.lattice[0]) % V.lattice[1], K = dof / (V.lattice[0] * V.lattice[1]);
    return I >= owned_lo[0] && J >= owned_lo[1] && K >= owned_lo[2];
  }
  /// facet tags under the cfg1 convention: global face x = lo -> 1, other global faces -> 2
  std::map<int, int> boundary_tags() const
  {
    std::map<int, int> tags;
    for (int f = 0; f < 6; ++f)
      if (face_tag[f]) tags[f] = face_tag[f];
    return tags;
  }
};

/// Weak-scaled box: n cells per direction PER RANK, global mesh (px nx, py ny, pz nz)
/// cells on [lo, hi].  periodic[a] identifies the upper face of axis a with the lower
/// one (a rank can then be its own neighbour).  Returned by pointer: V refers to mesh.
inline std::unique_ptr<BoxPartition> create_distributed_box(std::array<int, 3> n, int degree, int nproc, int rank,
                                                            std::array<double, 3> lo = {0, 0, 0},
                                                            std::array<double, 3> hi = {1, 1, 1},
                                                            std::array<bool, 3> periodic = {false, false, false})
{
  auto part = std::make_unique<BoxPartition>();
  BoxPartition& P = *part;
  const int per[3] = {periodic[0], periodic[1], periodic[2]};
  wf_box_partition_info info;
  check(wf_box_partition(n.data(), degree, nproc, rank, per, &info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  GhostLists& g = P.ghosts;
  g.send_neighbors.resize(7);
  g.recv_neighbors.resize(7);
  g.send_offsets.resize(8);
  g.recv_offsets.resize(8);
  g.send_indices.resize((std::size_t)info.num_send_indices);
  g.ghost_positions.resize((std::size_t)info.num_recv_indices);
  check(wf_box_partition(n.data(), degree, nproc, rank, per, &info, g.send_neighbors.data(), g.send_offsets.data(),
                         g.send_indices.data(), g.recv_neighbors.data(), g.recv_offsets.data(), g.ghost_positions.data()));
  g.send_neighbors.resize((std::size_t)info.num_send_neighbors);
  g.recv_neighbors.resize((std::size_t)info.num_recv_neighbors);
  g.send_offsets.resize((std::size_t)info.num_send_neighbors + 1);
  g.recv_offsets.resize((std::size_t)info.num_recv_neighbors + 1);
  P.rank = rank;
  P.degree = degree;
  P.n_local = n;
  P.periodic = periodic;
  P.size_global = info.size_global;
  P.owned_count = info.num_owned;
  std::array<double, 3> llo, lhi;
  for (int a = 0; a < 3; ++a) {
    P.procs[a] = info.procs[a];
    P.coords[a] = info.coords[a];
    P.owned_lo[a] = info.owned_lo[a];
    // the rank's slab of the global box, in global coordinates
    const double h = (hi[a] - lo[a]) / (P.procs[a] * n[a]);
    llo[a] = lo[a] + h * n[a] * P.coords[a];
    lhi[a] = lo[a] + h * n[a] * (P.coords[a] + 1);
  }
  for (int f = 0; f < 6; ++f) P.face_tag[f] = info.face_tag[f];
  P.mesh = create_box(n, llo, lhi);
  P.V = create_functionspace(P.mesh, degree, /*build_dofmap=*/false);
  g.ndofs = P.V.ndofs();
  return part;
}

/// demo/cpu_planar3d/main.cpp:48-66: (time step, steps per period) from mesh::h = the smallest cell diameter
inline std::pair<double, int> cfl_time_step(const BoxMesh& mesh, int degree, double c0, double freq, double CFL = 0.5)
{
  return cfl_time_step(mesh.nverts(), mesh.x.data(), mesh.ncells(), mesh.geom_dofmap.data(), degree, c0, freq, CFL);
}

}  // namespace wavehip
