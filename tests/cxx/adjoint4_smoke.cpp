// wf_leapfrog4_correlate through the C++ wrapper: seven vectors of 523 entries given by integer formulas, once with z and
// once without.  Prints one line per entry,
//   p <i> bits <16 hex digits>,   z <i> bits <16 hex digits>   and   q <i> bits <16 hex digits>   (q: p of the call without z)
// tests/test_gpu_adjoint4_kernels.py does the same in Python and compares bit for bit.  Every input is exact in binary.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "wavehip.hpp"

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
  const std::size_t N = 523;
  std::vector<double> hl(N), ho(N), hup(N), hu(N), hum(N), hw(N), hp(N);
  for (std::size_t i = 0; i < N; ++i) {
    hl[i] = (double)((i * 7919) % 1009) / 1024.0 - 0.5;
    ho[i] = (double)((i * 31337) % 1033) / 1024.0 - 0.5;
    hup[i] = (double)((i * 104729) % 1013) / 1024.0 - 0.25;
    hu[i] = (double)((i * 1299709) % 1019) / 1024.0 - 0.75;
    hum[i] = (double)((i * 15485863) % 1021) / 1024.0 - 0.5;
    hw[i] = (double)((i * 27644437) % 1039) / 1024.0 - 0.5;
    hp[i] = (double)((i * 611953) % 1031) / 1024.0 - 0.5;
  }
  array<double> lam(N), om(N), up(N), u(N), um(N), w(N), p(N), q(N), z(N);
  lam.set(hl);
  om.set(ho);
  up.set(hup);
  u.set(hu);
  um.set(hum);
  w.set(hw);
  p.set(hp);
  q.set(hp);
  z.set(std::vector<double>(N, -1.0));
  leapfrog4_correlate((std::int64_t)N, lam.data(), om.data(), up.data(), u.data(), um.data(), w.data(), p.data(), z.data());
  leapfrog4_correlate((std::int64_t)N, lam.data(), om.data(), up.data(), u.data(), um.data(), w.data(), q.data());
  check(wf_sync(nullptr));
  print_bits("p", p.copy_to_host());
  print_bits("z", z.copy_to_host());
  print_bits("q", q.copy_to_host());
  return 0;
}
