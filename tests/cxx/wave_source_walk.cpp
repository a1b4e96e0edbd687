// The plane source of the time loops (csrc/wave_source.h) evaluated on the host: plain C++17, no HIP, a program with
// its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_wave_source_host.py.
//
//   wave_source_walk CASES      CASES: one case per line, nine 64-bit words in hexadecimal -- the bits of c0, c0_squared,
//                               p0, w0, freq0, alpha, period and t, and the medium flag
// prints per case the bits of window(t), s1(t), s1_left_to_right(t) and s2(), so that the test compares them bit for bit
// with the expressions of the Python model.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "wave_source.h"

static double from_bits(uint64_t u)
{
  double x;
  std::memcpy(&x, &u, sizeof x);
  return x;
}

static uint64_t to_bits(double x)
{
  uint64_t u;
  std::memcpy(&u, &x, sizeof u);
  return u;
}

int main(int argc, char** argv)
{
  if (argc != 2) {
    std::fprintf(stderr, "usage: wave_source_walk CASES\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::fprintf(stderr, "wave_source_walk: cannot open %s\n", argv[1]);
    return 2;
  }
  uint64_t w[9];
  long cases = 0;
  while (std::fscanf(f, "%" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, &w[0],
                     &w[1], &w[2], &w[3], &w[4], &w[5], &w[6], &w[7], &w[8]) == 9) {
    const wf_wave_source p{from_bits(w[0]), from_bits(w[1]), from_bits(w[2]), from_bits(w[3]), from_bits(w[4]), from_bits(w[5]),
                           from_bits(w[6]), (int)w[8]};
    const double t = from_bits(w[7]);
    std::printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", to_bits(wf::wave_window(p, t)), to_bits(wf::wave_s1(p, t)),
                to_bits(wf::wave_s1_left_to_right(p, t)), to_bits(wf::wave_s2(p)));
    ++cases;
  }
  std::fclose(f);
  std::printf("%ld cases\n", cases);
  return 0;
}
