// Host-side launch plan of wf_tsmm (tsmm.hip; no device code, no HIP): how a product (ncells x K) . (K x N) is cut into
// launches -- column passes and row ranges -- and, per launch, the grid, the LDS table and the split between the
// straight-line main loop and the column-split tail of a partial last round.  tsmm.hip launches from these functions;
// tests/cxx/tsmm_plan_walk.cpp walks them on the host.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace wf {

// k-steps per chunk: the A operands of a chunk are loaded two chunks ahead (three rotating
// register sets), the B operands (LDS) one k-step ahead, so that no MFMA waits on the load
// issued just before it.  The LDS table is zero-padded to a whole number of chunks.
constexpr int kTsmmChunk = 8;
#ifndef WF_TSMM_WAVES
#define WF_TSMM_WAVES 8
#endif
constexpr int kTsmmWaves = WF_TSMM_WAVES;   // waves per workgroup (one workgroup per CU)
constexpr int kTsmmGrid = 256;              // workgroups of the persistent grid: one per CU
constexpr size_t kTsmmLdsLimit = 160 * 1024;

// Columns in passes of at most 128 (8 accumulator tiles of 16 per wave), the tiles spread evenly
// over the passes (N = 216: 7 + 7 tiles rather than 8 + 6 with two idle); table rows in ranges
// of at most 128 (the LDS-resident block is 128 x 144 doubles = 147 KB), whole 32-row chunks
// first, later ranges accumulating onto out.  The P5..P7 tables of demo/gpu_operator
// (216^2, 343^2, 512^2) take 4 / 9 / 16 launches.
struct TsmmSplit {
  int tiles, npass, tpp;   // column tiles of 16, passes, tiles per pass: pass i starts at column 16 tpp i
  int nk, kc;              // row ranges, rows per range: range j starts at row kc j
};

inline TsmmSplit tsmm_split(int K, int N)
{
  TsmmSplit s;
  s.tiles = (N + 15) / 16;
  s.npass = (s.tiles + 7) / 8;
  s.tpp = (s.tiles + s.npass - 1) / s.npass;
  s.nk = (K + 127) / 128;
  s.kc = 32 * (((K + s.nk - 1) / s.nk + 31) / 32);
  return s;
}

// column tiles of the pass that starts at column n0
inline int tsmm_pass_tiles(const TsmmSplit& s, int N, int n0) { return std::min(s.tpp, (N - n0 + 15) / 16); }

// the instantiation NT (accumulator tiles per wave) that serves a pass of nt column tiles: there is no k_tsmm<3>
inline int tsmm_kernel_nt(int nt) { return nt == 3 ? 4 : std::min(nt, 8); }

// The launches of one product in the order they are queued: column passes outermost, the row ranges of a pass in
// ascending order, so that the range with k0 > 0 (ACC) finds the sums of the ranges before it in out.
struct TsmmLaunch {
  int n0, nt, NT;   // first column, column tiles of the pass, the instantiation that serves them
  int k0, K;        // table rows [k0, k0 + K)
};

// f(launch) -> int for every launch; stops at, and returns, the first non-zero result
template <class F>
inline int tsmm_for_each_launch(int K, int N, F&& f)
{
  const TsmmSplit s = tsmm_split(K, N);
  for (int n0 = 0; n0 < N; n0 += 16 * s.tpp) {
    const int nt = tsmm_pass_tiles(s, N, n0);
    for (int k0 = 0; k0 < K; k0 += s.kc) {
      const int rc = f(TsmmLaunch{n0, nt, tsmm_kernel_nt(nt), k0, std::min(s.kc, K - k0)});
      if (rc != 0) return rc;
    }
  }
  return 0;
}

// One launch: rows [k0, k0 + K) of the table, NT column tiles, all cells.
struct TsmmLaunchPlan {
  int nch;              // chunks of kTsmmChunk k-steps (of 4 rows)
  int rows;             // table rows in LDS in use: 4 kTsmmChunk nch (+ 4 spare)
  int NP;               // row stride of the table in LDS, in doubles
  size_t lds;           // bytes
  unsigned nb;          // workgroups
  int64_t ntiles, rem;  // cell tiles of 16; those of a partial last round of the nb kTsmmWaves waves
  int64_t main_tiles;   // cell tiles [0, main_tiles) run in the main loop
  int tail_ct;          // 0: no tail; else the tiles [main_tiles, ntiles) run as units of tail_ct column tiles
};

inline TsmmLaunchPlan tsmm_launch_plan(int NT, int64_t ncells, int K)
{
  TsmmLaunchPlan p;
  const int KT = (K + 3) / 4;
  p.nch = (KT + kTsmmChunk - 1) / kTsmmChunk;
  p.rows = 4 * kTsmmChunk * p.nch;
  const int NW = 16 * NT;
  p.NP = NW + ((NW & 31) == 16 ? 0 : 16);
  p.lds = (size_t)(p.rows + 4) * p.NP * sizeof(double);
  p.ntiles = (ncells + 15) / 16;
  p.nb = (unsigned)std::min<int64_t>(p.ntiles, kTsmmGrid);   // one workgroup per CU; small problems spread over CUs first
  // partial last round: split its tiles along the columns when every wave then gets at most one unit
  const int64_t nwaves = (int64_t)p.nb * kTsmmWaves;
  p.rem = nwaves > 0 ? p.ntiles % nwaves : 0;
  p.main_tiles = p.ntiles;
  p.tail_ct = 0;
  if (p.rem > 0 && KT <= 4 * kTsmmChunk)
    for (int ct : {1, 2, 4})
      if (ct < NT && p.rem * ((NT + ct - 1) / ct) <= nwaves) {
        p.tail_ct = ct;
        p.main_tiles = p.ntiles - p.rem;
        break;
      }
  return p;
}

}  // namespace wf
