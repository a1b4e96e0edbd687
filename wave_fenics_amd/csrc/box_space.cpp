// Host side of the box path: what mesh::create_box + fem::create_functionspace give the reference's drivers
// (demo/gpu_operator/main.cpp:60-72) in this engine's lexicographic numbering, the collocated facet masses of the
// tagged box faces, and the Cartesian partition with its ghost lists (the idea of demo/gpu_cg/mesh.hpp:37-63).
// Host-only C ABI (wf_box_*, wf_decompose3d), used by the Python package (box.py, linear_gll.py, distributed.py) and by
// the C++ mirror (include/wavehip_box.hpp): neither wrapper holds a rule of its own.
#include <map>

#include "op.h"

using namespace wf;

namespace {

const char* box_sizes_error(const int* n)
{
  if (!n || n[0] < 1 || n[1] < 1 || n[2] < 1) return "n must be three positive cell counts";
  if (((int64_t)n[0] + 1) * ((int64_t)n[1] + 1) * ((int64_t)n[2] + 1) >= ((int64_t)1 << 31)) return "more than 2^31 vertices";
  return nullptr;
}

// the lattice (P n + 1 per axis) of a degree-P space on n cells; false if it has 2^31 points or more
bool box_lattice(int P, const int* n, int64_t* N)
{
  for (int a = 0; a < 3; ++a) N[a] = (int64_t)P * n[a] + 1;
  return N[0] * N[1] < ((int64_t)1 << 31) && N[0] * N[1] * N[2] < ((int64_t)1 << 31);
}

// One direction of the exchange with neighbour `nb`: per axis the lower plane (kind -1), the upper plane (+1) or the
// owned range (0) of the local lattice.
struct Segment {
  int nb;
  int kind[3];
};

// The lists of one side of the exchange: neighbours ascending, the segments of one neighbour in the order they were
// found.  Counts always; writes where the arrays are given.
void emit_segments(std::vector<Segment>& segs, const int* lattice, const int* owned_lo, int* neighbors, int32_t* offsets,
                   int32_t* indices, int* num_neighbors, int32_t* num_indices)
{
  std::stable_sort(segs.begin(), segs.end(), [](const Segment& a, const Segment& b) { return a.nb < b.nb; });
  int k = 0;
  int32_t m = 0;
  for (size_t s = 0; s < segs.size(); ++s) {
    if (s == 0 || segs[s].nb != segs[s - 1].nb) {
      if (neighbors) {
        neighbors[k] = segs[s].nb;
        offsets[k] = m;
      }
      ++k;
    }
    int b[3], e[3];
    for (int a = 0; a < 3; ++a) {
      const int kind = segs[s].kind[a], hi = lattice[a] - 1;
      b[a] = kind < 0 ? 0 : kind > 0 ? hi : owned_lo[a];
      e[a] = kind < 0 ? 0 : hi;
    }
    for (int K = b[2]; K <= e[2]; ++K)
      for (int J = b[1]; J <= e[1]; ++J)
        for (int I = b[0]; I <= e[0]; ++I, ++m)
          if (indices) indices[m] = (int32_t)(I + (int64_t)lattice[0] * (J + (int64_t)lattice[1] * K));
  }
  if (offsets) offsets[k] = m;
  *num_neighbors = k;
  *num_indices = m;
}

}  // namespace

// ---- the box as a dofmap mesh (box_mesh.h) ----
void wf::fill_box_dofmap(int P, int nx, int ny, int nz, int32_t* dofmap)
{
  const int n = P + 1, nd = n * n * n;
  const size_t NX = (size_t)P * nx + 1, NY = (size_t)P * ny + 1;
  for (int cz = 0; cz < nz; ++cz)
    for (int cy = 0; cy < ny; ++cy)
      for (int cx = 0; cx < nx; ++cx) {
        const size_t c = (size_t)cx + (size_t)nx * (cy + (size_t)ny * cz);
        const size_t base = (size_t)P * cx + NX * ((size_t)P * cy + NY * ((size_t)P * cz));
        for (int k = 0; k < n; ++k)
          for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) dofmap[c * nd + i + n * (j + n * k)] = (int32_t)(base + i + NX * (j + NY * k));
      }
}

void wf::fill_box_vertex_map(int nx, int ny, int nz, int32_t* geom_dofmap)
{
  const size_t ncells = (size_t)nx * ny * nz;
  for (size_t c = 0; c < ncells; ++c)
    for (int v = 0; v < 8; ++v) geom_dofmap[c * 8 + v] = (int32_t)box_vertex(nx, ny, c, v);
}

int wf::check_box_args(const char* who, int degree, int nx, int ny, int nz, const double* h_xverts)
{
  if (int rc = check_hex_degree(degree, who)) return rc;
  WF_REQUIRE(nx > 0 && ny > 0 && nz > 0 && h_xverts, std::string(who) + ": bad mesh");
  const size_t NX = (size_t)degree * nx + 1, NY = (size_t)degree * ny + 1, NZ = (size_t)degree * nz + 1;
  WF_REQUIRE(NX * NY * NZ < ((size_t)1 << 31), std::string(who) + ": dof lattice exceeds int32");
  return WF_OK;
}

wf::BoxDesc::BoxDesc(int kind, int P, int nx, int ny, int nz, const double* h_xverts, double c0, const double* h_cell_coeff,
                     int flags, const wf_tuning* tuning)
{
  const size_t ncells = (size_t)nx * ny * nz, nd = (size_t)(P + 1) * (P + 1) * (P + 1);
  dofmap.resize(ncells * nd);
  geom_dofmap.resize(ncells * 8);
  fill_box_dofmap(P, nx, ny, nz, dofmap.data());
  fill_box_vertex_map(nx, ny, nz, geom_dofmap.data());
  desc.kind = kind;
  desc.degree = P;
  desc.ncells = (int)ncells;
  desc.ndofs = (int)(((size_t)P * nx + 1) * ((size_t)P * ny + 1) * ((size_t)P * nz + 1));
  desc.h_dofmap = dofmap.data();
  desc.nverts = (nx + 1) * (ny + 1) * (nz + 1);
  desc.h_xverts = h_xverts;
  desc.h_geom_dofmap = geom_dofmap.data();
  desc.c0 = c0;
  desc.flags = flags;
  desc.tuning = tuning;
  desc.h_cell_coeff = h_cell_coeff;
}

extern "C" {

int wf_box_mesh(const int* n, const double* lo, const double* hi, double* h_x, int32_t* h_geom_dofmap)
{
  WF_REQUIRE(lo && hi && h_x && h_geom_dofmap, "wf_box_mesh: null argument");
  if (const char* bad = box_sizes_error(n)) {
    set_error(std::string("wf_box_mesh: ") + bad);
    return WF_ERR_INVALID;
  }
  const int nx = n[0], ny = n[1], nz = n[2];
  double step[3];
  for (int d = 0; d < 3; ++d) step[d] = (hi[d] - lo[d]) / n[d];
  size_t v = 0;
  for (int c = 0; c <= nz; ++c)
    for (int b = 0; b <= ny; ++b)
      for (int a = 0; a <= nx; ++a, ++v) {
        const int i[3] = {a, b, c};
        // numpy.linspace: lo + step * i, the last point exactly hi
        for (int d = 0; d < 3; ++d) h_x[v * 3 + d] = i[d] == n[d] ? hi[d] : lo[d] + step[d] * i[d];
      }
  fill_box_vertex_map(nx, ny, nz, h_geom_dofmap);
  return WF_OK;
}

int wf_box_dofmap(int degree, const int* n, int32_t* h_dofmap)
{
  WF_REQUIRE(degree >= 1 && degree <= kMaxDegree, "wf_box_dofmap: degree must be 1..7");
  int64_t N[3];
  WF_REQUIRE(!box_sizes_error(n) && box_lattice(degree, n, N), "wf_box_dofmap: n must be three positive cell counts, fewer than 2^31 dofs");
  WF_REQUIRE(h_dofmap, "wf_box_dofmap: null output");
  fill_box_dofmap(degree, n[0], n[1], n[2], h_dofmap);
  return WF_OK;
}

int wf_box_facet_mass(int degree, const int* n, const double* h_x, const int* face_tag, int tag, const double* h_cell_weight,
                      int64_t* nout, int32_t* h_idx, double* h_mass)
{
  WF_REQUIRE(degree >= 1 && degree <= kMaxDegree, "wf_box_facet_mass: degree must be 1..7");
  int64_t N[3];
  WF_REQUIRE(!box_sizes_error(n) && box_lattice(degree, n, N), "wf_box_facet_mass: n must be three positive cell counts, fewer than 2^31 dofs");
  WF_REQUIRE(tag != 0, "wf_box_facet_mass: tag 0 means untagged");
  WF_REQUIRE(h_x && face_tag && nout && !h_idx == !h_mass, "wf_box_facet_mass: null argument");
  const int P = degree, nx = n[0], ny = n[1];
  // the facets of the tagged faces: face 2 * axis + side in turn, over each the second tangential axis slowest
  std::vector<int32_t> cell, axis, side;
  for (int ax = 0; ax < 3; ++ax)
    for (int sd = 0; sd < 2; ++sd) {
      if (face_tag[2 * ax + sd] != tag) continue;
      const int ta = ax == 0 ? 1 : 0, tb = ax == 2 ? 1 : 2;
      int c[3];
      c[ax] = sd == 0 ? 0 : n[ax] - 1;
      for (c[tb] = 0; c[tb] < n[tb]; ++c[tb])
        for (c[ta] = 0; c[ta] < n[ta]; ++c[ta]) {
          cell.push_back((int32_t)(c[0] + (int64_t)nx * (c[1] + (int64_t)ny * c[2])));
          axis.push_back(ax);
          side.push_back(sd);
        }
    }
  FacetList facets{(int64_t)cell.size(), cell.data(), axis.data(), side.data()};
  auto vertex = [&](int64_t c, int v) { return (int64_t)box_vertex(nx, ny, (size_t)c, v); };
  auto dof = [&](int64_t c, const int* l) {
    const int64_t cx = c % nx, cy = (c / nx) % ny, cz = c / ((int64_t)nx * ny);
    return (int32_t)((P * cx + l[0]) + N[0] * ((P * cy + l[1]) + N[1] * (P * cz + l[2])));
  };
  std::map<int32_t, double> acc;
  if (int rc = facet_mass(P, facets, (int64_t)nx * ny * n[2], h_x, vertex, dof, h_cell_weight, acc)) return rc;
  *nout = (int64_t)acc.size();
  if (h_idx) {
    for (const auto& kv : acc) {
      *h_idx++ = kv.first;
      *h_mass++ = kv.second;
    }
  }
  return WF_OK;
}

int wf_decompose3d(int nproc, int* procs)
{
  WF_REQUIRE(nproc >= 1 && procs, "wf_decompose3d: nproc must be positive, procs not null");
  int best[3] = {nproc, 1, 1};
  for (int a = 1; a <= nproc; ++a) {
    if (nproc % a) continue;
    for (int b = 1; b <= nproc / a; ++b) {
      if ((nproc / a) % b) continue;
      int d[3] = {a, b, nproc / a / b};
      std::sort(d, d + 3, [](int x, int y) { return x > y; });
      // the most balanced split: smallest (d0 - d2, d0)
      if (d[0] - d[2] < best[0] - best[2] || (d[0] - d[2] == best[0] - best[2] && d[0] < best[0])) std::copy(d, d + 3, best);
    }
  }
  std::copy(best, best + 3, procs);
  return WF_OK;
}

int wf_box_partition(const int* n, int degree, int nproc, int rank, const int* periodic, wf_box_partition_info* info,
                     int* send_neighbors, int32_t* send_offsets, int32_t* send_indices, int* recv_neighbors,
                     int32_t* recv_offsets, int32_t* ghost_positions)
{
  WF_REQUIRE(info, "wf_box_partition: null info");
  WF_REQUIRE(degree >= 1 && degree <= kMaxDegree, "wf_box_partition: degree must be 1..7");
  int64_t N[3];
  WF_REQUIRE(!box_sizes_error(n) && box_lattice(degree, n, N), "wf_box_partition: n must be three positive cell counts, fewer than 2^31 local dofs");
  WF_REQUIRE(nproc >= 1 && rank >= 0 && rank < nproc, "wf_box_partition: rank must be in [0, nproc)");
  const bool fill = send_neighbors != nullptr;
  WF_REQUIRE(fill == !!send_offsets && fill == !!recv_neighbors && fill == !!recv_offsets && (fill || (!send_indices && !ghost_positions)),
             "wf_box_partition: pass all six arrays or none");
  wf_box_partition_info I{};
  wf_decompose3d(nproc, I.procs);
  const int* p = I.procs;
  // rank = rz + pz (ry + py rx): z fastest (compute_cartesian_indices)
  I.coords[0] = rank / (p[1] * p[2]);
  I.coords[1] = (rank / p[2]) % p[1];
  I.coords[2] = rank % p[2];
  I.size_global = I.num_owned = 1;
  bool per[3];
  for (int a = 0; a < 3; ++a) {
    per[a] = periodic && periodic[a];
    // a point shared by several ranks belongs to the lowest one: the lower plane is ghost wherever a lower neighbour
    // exists, which on a periodic axis is everywhere
    I.owned_lo[a] = (I.coords[a] > 0 || per[a]) ? 1 : 0;
    I.lattice[a] = (int)N[a];
    I.size_global *= (int64_t)degree * p[a] * n[a] + (per[a] ? 0 : 1);
    I.num_owned *= N[a] - I.owned_lo[a];
    // cfg1: global face x = lo carries tag 1, every other global face tag 2; interfaces and periodic faces none
    I.face_tag[2 * a] = (!per[a] && I.coords[a] == 0) ? (a == 0 ? 1 : 2) : 0;
    I.face_tag[2 * a + 1] = (!per[a] && I.coords[a] == p[a] - 1) ? 2 : 0;
  }
  std::vector<Segment> send, recv;
  for (int dx = 0; dx < 2; ++dx)
    for (int dy = 0; dy < 2; ++dy)
      for (int dz = 0; dz < 2; ++dz) {
        if (!dx && !dy && !dz) continue;
        const int d[3] = {dx, dy, dz};
        int up[3], dn[3];
        bool up_ok = true, dn_ok = true;
        for (int a = 0; a < 3; ++a) {
          up[a] = I.coords[a] + d[a];
          dn[a] = I.coords[a] - d[a];
          if (per[a]) {
            up[a] = (up[a] + p[a]) % p[a];
            dn[a] = (dn[a] + p[a]) % p[a];
          }
          up_ok = up_ok && up[a] >= 0 && up[a] < p[a];
          dn_ok = dn_ok && dn[a] >= 0 && dn[a] < p[a];
        }
        // the upper neighbour +d holds my upper planes as ghosts; the lower neighbour -d owns my lower planes
        if (up_ok) send.push_back({up[2] + p[2] * (up[1] + p[1] * up[0]), {dx, dy, dz}});
        if (dn_ok) recv.push_back({dn[2] + p[2] * (dn[1] + p[1] * dn[0]), {-dx, -dy, -dz}});
      }
  emit_segments(send, I.lattice, I.owned_lo, nullptr, nullptr, nullptr, &I.num_send_neighbors, &I.num_send_indices);
  emit_segments(recv, I.lattice, I.owned_lo, nullptr, nullptr, nullptr, &I.num_recv_neighbors, &I.num_recv_indices);
  if (fill) {
    WF_REQUIRE((send_indices || !I.num_send_indices) && (ghost_positions || !I.num_recv_indices), "wf_box_partition: pass all six arrays or none");
    emit_segments(send, I.lattice, I.owned_lo, send_neighbors, send_offsets, send_indices, &I.num_send_neighbors, &I.num_send_indices);
    emit_segments(recv, I.lattice, I.owned_lo, recv_neighbors, recv_offsets, ghost_positions, &I.num_recv_neighbors, &I.num_recv_indices);
  }
  *info = I;
  return WF_OK;
}

}  // extern "C"
