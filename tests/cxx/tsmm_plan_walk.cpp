// The launch plan of wf_tsmm (csrc/tsmm_plan.h, the header tsmm.hip launches from) walked on the host: plain C++17, no
// HIP, built by tests/test_tsmm_host.py under AddressSanitizer and UndefinedBehaviorSanitizer.
//
//   tsmm_plan_walk ncells K N [ncells K N ...]   one line per launch of each product:
//       launch ncells= Kfull= N= n0= NT= nt= k0= K= nch= acc= nb= ntiles= rem= main_tiles= tail_ct= rounds= units= cmod= lds=
//     rounds = most cell tiles a wave takes in the main loop, units = tail units per cell tile (0 without a tail),
//     cmod = ncells % 16 (cells of the partial last tile), lds in bytes
//   tsmm_plan_walk --exhaustive KMAX             every (K, N) in 1..KMAX x 1..KMAX: the launches' rectangles
//       rows [k0, k0 + K) x columns [n0, min(N, n0 + 16 NT)) lie inside [0, K) x [0, N), are pairwise disjoint and add up to
//       K N entries (so they tile the table exactly once); no table exceeds the LDS limit; every range is what the kernel
//       can take.  Prints "exhaustive ..." and "<n> failures".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tsmm_plan.h"

using namespace wf;

static int walk_product(int64_t ncells, int K, int N)
{
  return tsmm_for_each_launch(K, N, [&](const TsmmLaunch& l) -> int {
    const TsmmLaunchPlan p = tsmm_launch_plan(l.NT, ncells, l.K);
    const int64_t nwaves = (int64_t)p.nb * kTsmmWaves;
    const int64_t rounds = nwaves > 0 ? (p.main_tiles + nwaves - 1) / nwaves : 0;
    const int units = p.tail_ct > 0 ? (l.NT + p.tail_ct - 1) / p.tail_ct : 0;
    std::printf("launch ncells=%lld Kfull=%d N=%d n0=%d NT=%d nt=%d k0=%d K=%d nch=%d acc=%d nb=%u ntiles=%lld rem=%lld main_tiles=%lld "
                "tail_ct=%d rounds=%lld units=%d cmod=%d lds=%zu\n",
                (long long)ncells, K, N, l.n0, l.NT, l.nt, l.k0, l.K, p.nch, l.k0 > 0 ? 1 : 0, p.nb, (long long)p.ntiles, (long long)p.rem,
                (long long)p.main_tiles, p.tail_ct, (long long)rounds, units, (int)(ncells % 16), p.lds);
    return 0;
  });
}

struct Rect {
  int k0, k1, n0, n1;
};

static long exhaustive(int kmax)
{
  long failures = 0, launches = 0;
  size_t max_lds = 0;
  int max_launches = 0;
  auto fail = [&](const char* what, int K, int N, const TsmmLaunch& l) {
    if (++failures <= 20) std::printf("FAIL %s: K=%d N=%d n0=%d NT=%d nt=%d k0=%d kk=%d\n", what, K, N, l.n0, l.NT, l.nt, l.k0, l.K);
  };
  std::vector<Rect> rects;
  for (int K = 1; K <= kmax; ++K)
    for (int N = 1; N <= kmax; ++N) {
      rects.clear();
      int last_n0 = -1, last_k0 = -1;
      tsmm_for_each_launch(K, N, [&](const TsmmLaunch& l) -> int {
        const TsmmLaunchPlan p = tsmm_launch_plan(l.NT, 1000, l.K);
        max_lds = std::max(max_lds, p.lds);
        if (p.lds > kTsmmLdsLimit) fail("LDS", K, N, l);
        // what k_tsmm can take: an instantiation that exists and holds the pass, at most 4 chunks (the tail keeps
        // 4 kTsmmChunk k-steps in registers, RPT table rows per thread cover 4 chunks), ranges that start on a chunk
        if (!(l.NT == 1 || l.NT == 2 || (l.NT >= 4 && l.NT <= 8)) || l.nt < 1 || l.nt > l.NT) fail("NT", K, N, l);
        if (l.K < 1 || l.K > 4 * 4 * kTsmmChunk || p.nch < 1 || p.nch > 4 || l.k0 % (4 * kTsmmChunk) != 0) fail("range", K, N, l);
        if ((size_t)(p.rows + 4) * p.NP * sizeof(double) != p.lds || p.NP < 16 * l.NT || p.NP % 32 != 16) fail("table", K, N, l);
        // order: a pass's ranges ascending from k0 = 0, so that ACC launches find the earlier sums in out
        if (l.n0 != last_n0 ? l.k0 != 0 : l.k0 <= last_k0) fail("order", K, N, l);
        last_n0 = l.n0;
        last_k0 = l.k0;
        const Rect r{l.k0, l.k0 + l.K, l.n0, std::min(N, l.n0 + 16 * l.NT)};
        if (r.k0 < 0 || r.k1 > K || r.n0 < 0 || r.n1 > N || r.k0 >= r.k1 || r.n0 >= r.n1) fail("outside", K, N, l);
        if (l.n0 + 16 * l.nt < r.n1 && l.n0 + 16 * l.nt < N) fail("pass", K, N, l);
        for (const Rect& q : rects)
          if (r.k0 < q.k1 && q.k0 < r.k1 && r.n0 < q.n1 && q.n0 < r.n1) fail("covered twice", K, N, l);
        rects.push_back(r);
        return 0;
      });
      long area = 0;
      for (const Rect& q : rects) area += (long)(q.k1 - q.k0) * (q.n1 - q.n0);
      if (area != (long)K * N) fail("not covered", K, N, TsmmLaunch{0, 0, 0, 0, 0});
      launches += (long)rects.size();
      max_launches = std::max(max_launches, (int)rects.size());
    }
  std::printf("exhaustive kmax=%d products=%ld launches=%ld max_launches=%d max_lds=%zu lds_limit=%zu\n", kmax, (long)kmax * kmax, launches,
              max_launches, max_lds, kTsmmLdsLimit);
  return failures;
}

int main(int argc, char** argv)
{
  long failures = 0;
  if (argc == 3 && !std::strcmp(argv[1], "--exhaustive")) {
    failures = exhaustive(std::atoi(argv[2]));
  } else if (argc >= 4 && (argc - 1) % 3 == 0) {
    for (int i = 1; i + 2 < argc; i += 3) {
      const long long ncells = std::atoll(argv[i]);
      const int K = std::atoi(argv[i + 1]), N = std::atoi(argv[i + 2]);
      if (ncells < 1 || K < 1 || N < 1) {
        std::printf("FAIL bad triple %s %s %s\n", argv[i], argv[i + 1], argv[i + 2]);
        ++failures;
        continue;
      }
      failures += walk_product(ncells, K, N) != 0;
    }
  } else {
    std::fprintf(stderr, "usage: tsmm_plan_walk ncells K N [...] | --exhaustive KMAX\n");
    return 2;
  }
  std::printf("%ld failures\n", failures);
  return failures ? 1 : 0;
}
