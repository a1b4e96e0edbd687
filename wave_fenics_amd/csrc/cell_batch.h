// The shape of a cell batch, stated once for the column-thread batch kernels (stiffness_batch.hip, mass_batch.hip) and
// their launchers, and the degree dispatch of those launchers.
#pragma once
#include <type_traits>

#include "common.h"

namespace wf {

// A 256-thread workgroup takes CB = floor(256 / n^2) cells of degree P at once (P4: 10 cells, 250 of 256 lanes busy);
// thread t < NT owns the column (i, j, *) of cell t / n^2.  Flat loops over the batch's CB * nd element-local entries
// take NFLAT steps of 256.
template <int P>
struct CellBatch {
  static constexpr int n = P + 1, n2 = n * n, nd = n * n2;
  static constexpr int CB = 256 / n2, NT = CB * n2;
  static constexpr int NFLAT = (CB * nd + 255) / 256;
  // dynamic LDS of the stiffness batch kernels: the tiles U, Fr, Fs [CB][nd] and D [n][n]
  static constexpr size_t stiffness_lds_bytes = (size_t)(3 * CB * nd + n2) * sizeof(double);
  // batches of ncells cells: the grid of a one-batch-per-workgroup kernel
  static constexpr unsigned batches(int ncells) { return (unsigned)((ncells + CB - 1) / CB); }
};

// cells_per_batch (common.h) is the same number where host code has a run-time P
static_assert(cells_per_batch(1) == CellBatch<1>::CB && cells_per_batch(2) == CellBatch<2>::CB, "cells_per_batch");
static_assert(cells_per_batch(3) == CellBatch<3>::CB && cells_per_batch(4) == CellBatch<4>::CB, "cells_per_batch");
static_assert(cells_per_batch(5) == CellBatch<5>::CB && cells_per_batch(6) == CellBatch<6>::CB, "cells_per_batch");
static_assert(cells_per_batch(7) == CellBatch<7>::CB, "cells_per_batch");

// f(std::integral_constant<int, P>) for the degree P = 1..7; any other degree is the error `what`
template <class F>
int dispatch_degree(int P, const char* what, F&& f)
{
  switch (P) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
  }
  set_error(what);
  return WF_ERR_UNSUPPORTED;
}

}  // namespace wf
