// Cell forms through the C++ wrapper: on a P2 box with a two-value coefficient, the stiffness form with the geometry the
// library chooses (per cell: the box is rectilinear), the stiffness form on per-point geometry and the lumped-mass form,
// of two vectors given by integer formulas.  Prints one line per form and cell,
//   <name> geometry <wf_geometry_mode> cell <c> bits <e_c as 16 hex digits>
// tests/test_gpu_cell_form_model.py builds the same forms in Python and compares bit for bit.  Every input is exact in
// binary, so both sides hand the library the same bits.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "wavehip.hpp"

int main()
{
  using namespace wavehip;
  set_device(0);
  const int P = 2, nx = 9, ny = 3, nz = 5;
  // rectilinear, graded: spacing 0.75, 1.5, 0.75, ... along every axis; vertex (a, b, c) -> a + (nx+1)(b + (ny+1)c)
  auto coord = [](int i) { return 0.75 * i + 0.75 * (i / 2); };
  std::vector<double> xv;
  for (int c = 0; c <= nz; ++c)
    for (int b = 0; b <= ny; ++b)
      for (int a = 0; a <= nx; ++a) {
        xv.push_back(coord(a));
        xv.push_back(coord(b));
        xv.push_back(coord(c));
      }
  std::vector<double> coeff;
  for (int cz = 0; cz < nz; ++cz)
    for (int cy = 0; cy < ny; ++cy)
      for (int cx = 0; cx < nx; ++cx) coeff.push_back(cx + cz < 5 ? 1.0 : 8.0);
  wf_tuning per_point{};
  per_point.geometry = WF_GEOMETRY_PER_POINT;
  CellForm<double> K(WF_OP_STIFFNESS, P, nx, ny, nz, xv.data(), 1500.0, nullptr, coeff.data());
  CellForm<double> Kp(WF_OP_STIFFNESS, P, nx, ny, nz, xv.data(), 1500.0, &per_point, coeff.data());
  CellForm<double> M(WF_OP_MASS_LUMPED, P, nx, ny, nz, xv.data(), 0.0, nullptr, coeff.data());
  const std::size_t N = (std::size_t)(P * nx + 1) * (P * ny + 1) * (P * nz + 1), nc = (std::size_t)nx * ny * nz;
  std::vector<double> hu(N), hl(N);
  for (std::size_t i = 0; i < N; ++i) {
    hu[i] = (double)((i * 7919) % 1009) / 1024.0 - 0.5;
    hl[i] = (double)((i * 104729) % 1013) / 1024.0 + 0.5;
  }
  array<double> u(N), lam(N);
  u.set(hu);
  lam.set(hl);
  const CellForm<double>* forms[3] = {&K, &Kp, &M};
  const char* names[3] = {"stiffness", "stiffness_point", "lumped"};
  for (int k = 0; k < 3; ++k) {
    if (forms[k]->num_cells() != nc || !forms[k]->cell_coeff()) return 2;
    array<double> out(nc);
    forms[k]->eval(lam.data(), u.data(), out.data());
    check(wf_sync(nullptr));
    const std::vector<double> he = out.copy_to_host();
    for (std::size_t c = 0; c < nc; ++c) {
      std::uint64_t b;
      std::memcpy(&b, &he[c], sizeof b);
      std::printf("%s geometry %d cell %zu bits %016" PRIx64 "\n", names[k], forms[k]->geometry(), c, b);
    }
  }
  return 0;
}
