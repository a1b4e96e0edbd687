// The two adjoint passes through the C++ wrapper: on a P3 box of 3 x 2 x 2 cells, three sources (two in one cell, one on
// a node) loaded with device values by Sources::add_values, and leapfrog_correlate over five vectors given by integer
// formulas.  Prints one line per dof,
//   b <i> bits <16 hex digits>      and      p <i> bits <16 hex digits>
// tests/test_gpu_adjoint_kernels.py does the same in Python and compares bit for bit.  Every input is exact in binary.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "wavehip.hpp"
#include "wavehip_box.hpp"

static void print_bits(const char* name, const std::vector<double>& v)
{
  for (std::size_t i = 0; i < v.size(); ++i) {
    std::uint64_t b;
    std::memcpy(&b, &v[i], sizeof b);
    std::printf("%s %zu bits %016" PRIx64 "\n", name, i, b);
  }
}

int main()
{
  using namespace wavehip;
  set_device(0);
  const int P = 3;
  const BoxMesh mesh = create_box({3, 2, 2}, {0, 0, 0}, {3, 2, 2});
  const BoxSpace V = create_functionspace(mesh, P);
  const std::size_t N = (std::size_t)V.ndofs();
  // (0.5, 0.25, 0.75) and (0.75, 0.5, 0.25) share cell 0; (1, 1, 1) is a vertex of the mesh, hence a node
  const std::vector<std::array<double, 3>> xyz = {{0.5, 0.25, 0.75}, {0.75, 0.5, 0.25}, {1.0, 1.0, 1.0}};
  const Sources src(V.space(), xyz, {ricker(1.0, 0.0, 0.0), ricker(1.0, 0.0, 0.0), ricker(1.0, 0.0, 0.0)});
  std::vector<double> hb(N), hl(N), hup(N), hu(N), hum(N), hp(N);
  for (std::size_t i = 0; i < N; ++i) {
    hb[i] = (double)((i * 31) % 17) / 16.0 - 0.5;
    hl[i] = (double)((i * 7919) % 1009) / 1024.0 - 0.5;
    hup[i] = (double)((i * 104729) % 1013) / 1024.0 - 0.25;
    hu[i] = (double)((i * 1299709) % 1019) / 1024.0 - 0.75;
    hum[i] = (double)((i * 15485863) % 1021) / 1024.0 - 0.5;
    hp[i] = (double)((i * 611953) % 1031) / 1024.0 - 0.5;
  }
  array<double> b(N), lam(N), up(N), u(N), um(N), p(N), vals(3);
  b.set(hb);
  lam.set(hl);
  up.set(hup);
  u.set(hu);
  um.set(hum);
  p.set(hp);
  vals.set(std::vector<double>{0.625, -1.75, 3.0});
  src.add_values(vals.data(), b.data(), -2.5);
  leapfrog_correlate((std::int64_t)N, lam.data(), up.data(), u.data(), um.data(), p.data());
  check(wf_sync(nullptr));
  print_bits("b", b.copy_to_host());
  print_bits("p", p.copy_to_host());
  return 0;
}
