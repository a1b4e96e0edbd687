// Walks the host-only box entries (csrc/box_space.cpp with function_space.cpp and tables.cpp) over the partition and
// facet-mass cases of tests/test_box_host.py, each with the size-only call followed by the fill call into arrays of
// exactly the reported sizes, and builds the box description of csrc/box_mesh.h at four (degree, box) pairs, compared
// entry by entry with wf_box_dofmap, wf_box_mesh and box_vertex.  Built as a stand-alone program with -fsanitize=address,undefined by
// tests/test_box_host.py::test_box_space_sanitized: the sanitizers see every read and write of the library code.
// Prints one checksum line; exit status 0 when every call returned what it should.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "box_mesh.h"
#include "wavehip.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("line %d: %s: %s\n", __LINE__, #cond, wf_last_error()); \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static long long walk_partition(int world, const int* n, int p, const int* per)
{
  long long sum = 0;
  for (int rank = 0; rank < world; ++rank) {
    wf_box_partition_info info;
    EXPECT(wf_box_partition(n, p, world, rank, per, &info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == WF_OK);
    std::vector<int> snb(7), rnb(7);
    std::vector<std::int32_t> soff(8), roff(8), sidx((std::size_t)info.num_send_indices), ridx((std::size_t)info.num_recv_indices);
    EXPECT(wf_box_partition(n, p, world, rank, per, &info, snb.data(), soff.data(), sidx.data(), rnb.data(), roff.data(),
                            ridx.data()) == WF_OK);
    EXPECT(soff[info.num_send_neighbors] == info.num_send_indices && roff[info.num_recv_neighbors] == info.num_recv_indices);
    const long long ndofs = (long long)info.lattice[0] * info.lattice[1] * info.lattice[2];
    for (std::int32_t v : sidx) {
      EXPECT(v >= 0 && v < ndofs);
      sum += v;
    }
    for (std::int32_t v : ridx) {
      EXPECT(v >= 0 && v < ndofs);
      sum += v;
    }
    sum += info.num_owned + info.size_global;
  }
  return sum;
}

static double walk_facets(const int* n, int p, bool weighted)
{
  const std::size_t nverts = (std::size_t)(n[0] + 1) * (n[1] + 1) * (n[2] + 1), ncells = (std::size_t)n[0] * n[1] * n[2];
  const double lo[3] = {0.1, -0.3, 0.0}, hi[3] = {1.3, 0.9, 2.0};
  std::vector<double> x(nverts * 3), weight(ncells);
  std::vector<std::int32_t> gd(ncells * 8), dm(ncells * (p + 1) * (p + 1) * (p + 1));
  EXPECT(wf_box_mesh(n, lo, hi, x.data(), gd.data()) == WF_OK);
  EXPECT(wf_box_dofmap(p, n, dm.data()) == WF_OK);
  for (std::size_t c = 0; c < ncells; ++c) weight[c] = 0.5 + 0.25 * (double)(c % 5);
  // displace the interior vertices a little: no facet stays a rectangle's neighbour
  for (int c = 1; c < n[2]; ++c)
    for (int b = 1; b < n[1]; ++b)
      for (int a = 1; a < n[0]; ++a) x[3 * (a + (std::size_t)(n[0] + 1) * (b + (std::size_t)(n[1] + 1) * c)) + (a + b + c) % 3] += 0.03;
  const int face_tag[6] = {1, 2, 2, 2, 2, 2};
  double sum = 0.0;
  for (int tag = 1; tag <= 2; ++tag) {
    std::int64_t nout = 0, nfill = 0;
    const double* w = weighted ? weight.data() : nullptr;
    EXPECT(wf_box_facet_mass(p, n, x.data(), face_tag, tag, w, &nout, nullptr, nullptr) == WF_OK);
    std::vector<std::int32_t> idx((std::size_t)nout);
    std::vector<double> m((std::size_t)nout);
    EXPECT(wf_box_facet_mass(p, n, x.data(), face_tag, tag, w, &nfill, idx.data(), m.data()) == WF_OK && nfill == nout);
    // the file path on the same facets
    std::vector<std::int32_t> cell, axis, side;
    for (int f = 0; f < 6; ++f) {
      if (face_tag[f] != tag) continue;
      const int ax = f / 2, ta = ax == 0 ? 1 : 0, tb = ax == 2 ? 1 : 2;
      int c[3];
      c[ax] = f % 2 ? n[ax] - 1 : 0;
      for (c[tb] = 0; c[tb] < n[tb]; ++c[tb])
        for (c[ta] = 0; c[ta] < n[ta]; ++c[ta]) {
          cell.push_back(c[0] + n[0] * (c[1] + n[1] * c[2]));
          axis.push_back(ax);
          side.push_back(f % 2);
        }
    }
    std::vector<std::int32_t> fidx(cell.size() * (p + 1) * (p + 1));
    std::vector<double> fm(fidx.size());
    std::int64_t nfile = 0;
    EXPECT(wf_fs_facet_mass_weighted(p, (std::int64_t)nverts, x.data(), (std::int64_t)ncells, gd.data(), dm.data(),
                                     (std::int64_t)cell.size(), cell.data(), axis.data(), side.data(), w, &nfile, fidx.data(),
                                     fm.data()) == WF_OK);
    EXPECT(nfile == nout);
    for (std::int64_t i = 0; i < nout && i < nfile; ++i) {
      EXPECT(idx[i] == fidx[i] && m[i] == fm[i]);
      sum += m[i];
    }
  }
  double h = 0.0;
  EXPECT(wf_fs_min_cell_diameter((std::int64_t)nverts, x.data(), (std::int64_t)ncells, gd.data(), &h) == WF_OK && h > 0.0);
  return sum + h;
}

// The box as a dofmap mesh (csrc/box_mesh.h): the description the box entry points hand to the dofmap entry points,
// entry by entry against wf_box_dofmap, wf_box_mesh and box_vertex, and every field of its descriptor.
static long long walk_box_desc(int p, int nx, int ny, int nz)
{
  const int n[3] = {nx, ny, nz}, nd = (p + 1) * (p + 1) * (p + 1);
  const std::size_t ncells = (std::size_t)nx * ny * nz, nverts = (std::size_t)(nx + 1) * (ny + 1) * (nz + 1);
  const double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {1.0, 2.0, 3.0};
  std::vector<double> x(nverts * 3), coeff(ncells, 1.5);
  std::vector<std::int32_t> gd(ncells * 8), dm(ncells * nd);
  EXPECT(wf_box_mesh(n, lo, hi, x.data(), gd.data()) == WF_OK);
  EXPECT(wf_box_dofmap(p, n, dm.data()) == WF_OK);
  EXPECT(wf::check_box_args("walk", p, nx, ny, nz, x.data()) == WF_OK);
  wf_tuning tun{};
  const wf::BoxDesc box(WF_OP_MASS_LUMPED, p, nx, ny, nz, x.data(), 1500.0, coeff.data(), WF_FLAG_ORDERED, &tun);
  const wf_op_desc& d = box.desc;
  EXPECT(box.dofmap.size() == dm.size() && box.geom_dofmap.size() == gd.size());
  EXPECT(d.h_dofmap == box.dofmap.data() && d.h_geom_dofmap == box.geom_dofmap.data() && d.h_xverts == x.data());
  EXPECT(d.kind == WF_OP_MASS_LUMPED && d.degree == p && d.ncells == (int)ncells && d.nverts == (int)nverts);
  EXPECT(d.ndofs == (p * nx + 1) * (p * ny + 1) * (p * nz + 1));
  EXPECT(d.c0 == 1500.0 && d.flags == WF_FLAG_ORDERED && d.tuning == &tun && d.h_cell_coeff == coeff.data());
  EXPECT(!d.h_perm && !d.h_G && !d.h_detJ && d.nq1 == 0 && !d.h_phi1 && !d.h_qpts1 && !d.h_qwts1);
  long long sum = 0;
  for (std::size_t e = 0; e < dm.size() && e < box.dofmap.size(); ++e) {
    EXPECT(box.dofmap[e] == dm[e] && dm[e] >= 0 && dm[e] < d.ndofs);
    sum += box.dofmap[e];
  }
  for (std::size_t c = 0; c < ncells && 8 * c < box.geom_dofmap.size(); ++c)
    for (int v = 0; v < 8; ++v) {
      const std::int32_t got = box.geom_dofmap[c * 8 + v];
      EXPECT(got == gd[c * 8 + v] && got == (std::int32_t)wf::box_vertex(nx, ny, c, v) && got >= 0 && got < d.nverts);
      sum += got;
    }
  return sum;
}

int main()
{
  const int cases[][8] = {  // world, nx, ny, nz, degree, periodic x y z
      {1, 2, 2, 2, 2, 1, 0, 0}, {1, 2, 1, 2, 3, 1, 1, 1}, {2, 2, 2, 1, 2, 1, 1, 0}, {4, 1, 2, 2, 2, 0, 0, 0}, {8, 1, 2, 1, 2, 0, 0, 0},
      {8, 1, 1, 1, 3, 1, 0, 1}, {6, 2, 1, 1, 1, 0, 1, 0}, {4, 1, 2, 2, 2, 1, 1, 1}, {8, 1, 1, 1, 2, 1, 0, 1}, {2, 2, 2, 2, 1, 0, 1, 0},
      {1, 2, 3, 1, 2, 0, 0, 0}, {7, 1, 2, 1, 2, 0, 0, 0}, {12, 1, 1, 2, 2, 0, 0, 0}, {12, 1, 1, 1, 1, 1, 1, 1}, {2, 2, 1, 2, 3, 1, 0, 0},
      {1, 1, 1, 1, 1, 0, 0, 0}, {1, 1, 1, 1, 1, 1, 1, 1}, {8, 1, 1, 1, 1, 0, 0, 0}, {3, 2, 1, 1, 7, 0, 0, 1}};
  long long isum = 0;
  for (const auto& c : cases) isum += walk_partition(c[0], c + 1, c[4], c + 5);
  const int boxes[][4] = {{3, 2, 4, 1}, {3, 2, 4, 2}, {2, 3, 2, 3}, {2, 2, 2, 4}, {1, 2, 3, 5}, {2, 1, 2, 6}, {2, 2, 1, 7}, {1, 1, 1, 1}};
  double fsum = 0.0;
  for (const auto& b : boxes)
    for (int weighted = 0; weighted < 2; ++weighted) fsum += walk_facets(b, b[3], weighted != 0);
  const int descs[][4] = {{1, 1, 1, 1}, {2, 2, 1, 3}, {4, 1, 2, 2}, {7, 1, 1, 2}};   // degree, nx, ny, nz
  long long dsum = 0;
  for (const auto& b : descs) dsum += walk_box_desc(b[0], b[1], b[2], b[3]);
  EXPECT(wf::check_box_args("walk", 8, 1, 1, 1, &fsum) == WF_ERR_UNSUPPORTED);
  EXPECT(wf::check_box_args("walk", 2, 1, 0, 1, &fsum) == WF_ERR_INVALID && wf::check_box_args("walk", 2, 1, 1, 1, nullptr) == WF_ERR_INVALID);
  EXPECT(wf::check_box_args("walk", 2, 2, 1, 1 << 30, &fsum) == WF_ERR_INVALID);
  // refusals leave the outputs alone
  wf_box_partition_info info;
  const int n[3] = {2, 2, 2}, zero[3] = {2, 0, 2};
  EXPECT(wf_box_partition(n, 2, 4, 4, nullptr, &info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == WF_ERR_INVALID);
  EXPECT(wf_box_partition(zero, 2, 4, 0, nullptr, &info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == WF_ERR_INVALID);
  EXPECT(wf_box_partition(n, 9, 4, 0, nullptr, &info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == WF_ERR_INVALID);
  EXPECT(wf_box_partition(n, 2, 4, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == WF_ERR_INVALID);
  std::printf("partition checksum %lld, facet checksum %.17g, box description checksum %lld, %d failures\n", isum, fsum, dsum,
              failures);
  return failures ? 1 : 0;
}
