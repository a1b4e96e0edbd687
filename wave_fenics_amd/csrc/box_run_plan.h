// Host-side plan of the z segmentation of the box marching kernels (box_run_plan.cpp; no device code, no HIP).
//
// Cost unit: layers.  A work item of L layers costs L + prologue (pipeline fill); the resident workgroups are slots that
// take the items in launch order as they free up (list scheduling).  The uniform plan cuts every column into equal
// segments; the run plan (owner form, DESIGN §4.2 "r19") gives every workgroup one run (col, z0, z1) of its own length.
#pragma once
#include <cstdint>
#include <vector>

namespace wf {

constexpr int kXcds = 8;   // workgroup b runs on XCD b mod 8 (as hard-wired in k_stiffness_owner's uniform order)
// prologue of a work item in layers: the guess every uniform cut is chosen with.  The owner form's run plan is priced
// with the same guess: the lz sweep of the P4 owner apply that was to replace it does not follow a + b rounds lz +
// c rounds (fitted c / b = 0.55 and -0.24 layers in two sweeps, residual 3 us on 55; profiles/r19_summary.md)
constexpr double kMarchPrologue = 1.5;
constexpr double kOwnerPrologue = kMarchPrologue;

struct BoxRun {
  int32_t col, z0, z1;   // layers [z0, z1) of column col (position in the column sequence the plan was made for)
};

struct BoxRunPlan {
  int uniform_lz = 0;          // layers per segment of the uniform plan (box_uniform_lz with kMarchPrologue, or wf_tuning.lz)
  double uniform_cost = 0.0;   // rounds * (uniform_lz + prologue)
  std::vector<BoxRun> runs;    // run table in launch order: entry e is the run of workgroup e; empty: the uniform plan stays
  double cost = 0.0;           // modelled makespan of the plan that runs
  int longest = 0;             // longest run in layers (uniform_lz when the uniform plan stays)
};

// the segment length that minimises rounds * (lz + prologue) over equal cuts of at least 3 layers
int box_uniform_lz(int ncols, int nz, long resident, double prologue, double* cost, long* items);

// Makespan of runs[e], e = xcd, xcd + nxcd, ..., started in that order on `slots` slots.
double box_runs_makespan(const std::vector<BoxRun>& runs, int xcd, int nxcd, int slots, double prologue);

// Uniform plan, and the run table when one is strictly better in the model.  lz_tuning > 0 (wf_tuning.lz) keeps the
// uniform plan, as does a uniform plan of one round whose columns are cut (or have fewer than 6 layers to cut).
BoxRunPlan box_run_plan(int ncols, int nz, int resident, int nxcd, double prologue, int lz_tuning);

// ---- run tables as the kernel takes them: [runs][3] = (column, z0, z1), entry e the run of workgroup e ----
// Aligned cut: every column cut at the same nseg places (lengths differ by at most one layer), the runs in segment-major
// order and dealt to the XCDs in contiguous chunks, as the uniform order deals its items: neighbouring columns march
// through the same layers at the same time, and what one reads as halo the other has just brought into the XCD's L2.
std::vector<int32_t> aligned_runs(int ncols, int nz, int nseg);
// What creation decides before it times anything (tune_owner_runs, op_create_box.hip; DESIGN §4.2 "r19"):
// whether the cut of the owner apply is chosen by timing at all: only at P4, where the bits of y do not depend on the
// cut, without wf_tuning.lz, and where the uniform plan (ncols columns in segments of lz layers) needs more than one
// round of the resident workgroups;
bool owner_cut_is_timed(int P, int tuning_lz, int ncols, int nz, int lz, long resident);
// and the nseg of the aligned_runs tables timed against the uniform plan: cuts of 4 to 12 layers per run, at most 17 of
// them, ascending (none where nz < 8).
std::vector<int> owner_cut_candidates(int nz);
// layers of the longest run of a table (0 for the empty table)
int longest_run(const std::vector<int32_t>& table);
// The kernel trusts its table: every run non-empty and inside its column, every (column, layer) exactly once.  The
// empty table (nruns = 0: the uniform plan runs) is valid.  The first fault found, runs in table order:
enum class RunTableFault : int { none = 0, outside_or_empty, covered_twice, not_covered };
RunTableFault check_run_table(const int32_t* runs, int32_t nruns, int ncols, int nz);

}  // namespace wf
