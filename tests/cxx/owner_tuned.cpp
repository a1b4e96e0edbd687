// The owner-computes separable box stiffness at P5 to P7 through the C ABI: wf_op_create_box (the default operator:
// k-split kernel, per-point geometry) against wf_op_create_box_tuned with wf_tuning.update = WF_UPDATE_OWNER on the same
// rectilinear box.  Checks the wf_op_info fields of both, applies both to one seeded x and prints
// max|dy| / max|y| per degree; "failures: N", exit status non-zero unless every degree is <= 1e-12.
// Run by tests/test_gpu_owner_high_degree.py on the GPU box.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "wavehip.hpp"

int main()
{
  using namespace wavehip;
  set_device(0);
  int failures = 0;
  for (int P = 5; P <= 7; ++P) {
    const int nx = 6, ny = 5, nz = 4;
    // rectilinear, graded: vertex (a, b, c) -> a + (nx+1)(b + (ny+1)c)
    std::mt19937_64 rng(100 + P);
    std::uniform_real_distribution<double> sp(0.5, 2.0), u(-1.0, 1.0);
    std::vector<double> ax[3];
    const int nn[3] = {nx, ny, nz};
    for (int d = 0; d < 3; ++d) {
      ax[d].push_back(0.0);
      for (int c = 0; c < nn[d]; ++c) ax[d].push_back(ax[d].back() + sp(rng));
    }
    std::vector<double> xv;
    for (int c = 0; c <= nz; ++c)
      for (int b = 0; b <= ny; ++b)
        for (int a = 0; a <= nx; ++a) {
          xv.push_back(ax[0][a]);
          xv.push_back(ax[1][b]);
          xv.push_back(ax[2][c]);
        }
    wf_op *dflt = nullptr, *own = nullptr;
    check(wf_op_create_box(WF_OP_STIFFNESS, P, nx, ny, nz, xv.data(), 1500.0, WF_FLAG_NONE, &dflt));
    wf_tuning tun{};
    tun.update = WF_UPDATE_OWNER;
    check(wf_op_create_box_tuned(WF_OP_STIFFNESS, P, nx, ny, nz, xv.data(), 1500.0, WF_FLAG_NONE, &tun, &own));
    wf_op_info_t id{}, io{};
    check(wf_op_info(dflt, &id));
    check(wf_op_info(own, &io));
    const double nd = (P + 1.0) * (P + 1.0) * (P + 1.0), ncells = (double)nx * ny * nz;
    const bool info_ok = id.kernel == WF_KERNEL_MARCH_BOX && id.geometry == WF_GEOMETRY_PER_POINT && id.metric == WF_METRIC_NONE &&
                         id.update == WF_UPDATE_NONE && io.kernel == WF_KERNEL_MARCH_BOX && io.geometry == WF_GEOMETRY_PER_CELL &&
                         io.metric == WF_METRIC_AXES && io.update == WF_UPDATE_OWNER && io.ndofs == id.ndofs && io.plan_lz > 0 &&
                         io.alg_bytes == ncells * (48.0 + 4.0 * nd) + 16.0 * io.ndofs && io.device_bytes < id.device_bytes;
    const std::size_t N = (std::size_t)io.ndofs;
    std::vector<double> hx(N), hy(N);
    for (auto& v : hx) v = u(rng);
    for (auto& v : hy) v = 1e6 * u(rng);
    array<double> x(N), y0(N), y1(N);
    x.set(hx);
    y0.set(hy);
    y1.set(hy);
    check(wf_op_apply(dflt, x.data(), y0.data(), nullptr));
    check(wf_op_apply(own, x.data(), y1.data(), nullptr));
    check(wf_sync(nullptr));
    const std::vector<double> r0 = y0.copy_to_host(), r1 = y1.copy_to_host();
    double dmax = 0.0, ymax = 0.0;
    bool finite = true;
    for (std::size_t i = 0; i < N; ++i) {
      finite = finite && std::isfinite(r1[i]);
      dmax = std::max(dmax, std::abs(r1[i] - r0[i]));
      ymax = std::max(ymax, std::abs(r0[i]));
    }
    const double err = dmax / ymax;
    const bool ok = info_ok && finite && err <= 1e-12;
    std::printf("P%d: info %s, owner vs default max|dy|/max|y| = %.3e %s\n", P, info_ok ? "ok" : "WRONG", err, ok ? "" : "FAIL");
    failures += ok ? 0 : 1;
    wf_op_destroy(dflt);
    wf_op_destroy(own);
  }
  std::printf("failures: %d\n", failures);
  return failures == 0 ? 0 : 1;
}
