// Cell coefficients through the C++ wrappers: a box stiffness operator (P4: the owner form) and a box lumped mass with a
// two-value coefficient, applied to a vector given by an integer formula.  Prints one line per operator,
//   <name> cell_coeff <0|1> checksum <sum_i y_i w_i> scale <sum_i |y_i w_i|>
// with 17 significant digits; tests/test_gpu_medium_model.py builds the same operators in Python and compares.
// Every input is exact in binary, so both sides hand the library the same bits.
#include <cmath>
#include <cstdio>
#include <vector>

#include "wavehip.hpp"

int main()
{
  using namespace wavehip;
  set_device(0);
  const int P = 4, nx = 9, ny = 3, nz = 5;
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
  // two layers: 1 in the cells cx + cz < 5, 8 elsewhere (an oblique interface: no block, column or segment boundary)
  std::vector<double> coeff;
  for (int cz = 0; cz < nz; ++cz)
    for (int cy = 0; cy < ny; ++cy)
      for (int cx = 0; cx < nx; ++cx) coeff.push_back(cx + cz < 5 ? 1.0 : 8.0);
  BoxStiffnessOperator<double> K(P, nx, ny, nz, xv.data(), 1500.0, nullptr, coeff.data());
  BoxMassOperatorLumped<double> M(P, nx, ny, nz, xv.data(), WF_FLAG_NONE, coeff.data());
  const std::size_t N = (std::size_t)(P * nx + 1) * (P * ny + 1) * (P * nz + 1);
  std::vector<double> hx(N), w(N);
  for (std::size_t i = 0; i < N; ++i) {
    hx[i] = (double)((i * 7919) % 1009) / 1024.0 - 0.5;
    w[i] = (double)((i * 104729) % 1013) / 1024.0 + 0.5;
  }
  array<double> x(N);
  x.set(hx);
  detail::OpBase* ops[2] = {&K, &M};
  const char* names[2] = {"stiffness", "lumped"};
  for (int k = 0; k < 2; ++k) {
    array<double> y(N);
    check(wf_memset(y.data(), 0, N * sizeof(double), nullptr));
    ops[k]->apply(x.data(), y.data());
    check(wf_sync(nullptr));
    const std::vector<double> hy = y.copy_to_host();
    double sum = 0.0, scale = 0.0;
    for (std::size_t i = 0; i < N; ++i) {
      sum += hy[i] * w[i];
      scale += std::abs(hy[i] * w[i]);
    }
    std::printf("%s cell_coeff %d checksum %.17e scale %.17e\n", names[k], ops[k]->cell_coeff() ? 1 : 0, sum, scale);
  }
  return 0;
}
