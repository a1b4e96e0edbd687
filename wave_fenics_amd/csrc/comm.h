// Internal declarations of the ghost exchange: the run-time binding of librccl and the communicator (comm.hip),
// shared with the updater (updater.hip) and the solver that reduces over owned entries (cg.hip).
#pragma once
#include "device_array.h"

namespace wf {

// the slice of the RCCL ABI used here (rccl.h of ROCm 7.x; values are part of the stable NCCL ABI)
typedef struct ncclComm* ncclComm_t;
typedef struct {
  char internal[128];
} ncclUniqueId;
enum { kNcclSuccess = 0, kNcclFloat64 = 8, kNcclSum = 0, kNcclMax = 2 };

struct RcclApi {
  void* handle = nullptr;
  std::string path;
  int (*GetVersion)(int*) = nullptr;
  int (*GetUniqueId)(ncclUniqueId*) = nullptr;
  int (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  int (*CommDestroy)(ncclComm_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*Send)(const void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};

// Loads librccl once; null (with the error set) if no candidate has every symbol.
RcclApi* rccl();

#define WF_NCCL_CHECK(api, expr)                                                              \
  do {                                                                                        \
    int _r = (expr);                                                                          \
    if (_r != ::wf::kNcclSuccess) {                                                           \
      ::wf::set_error(std::string(#expr) + " failed: " + (api)->GetErrorString(_r));           \
      return WF_ERR_COMM;                                                                     \
    }                                                                                         \
  } while (0)

}  // namespace wf

struct wf_comm {
  wf::ncclComm_t comm = nullptr;
  int rank = 0, nranks = 1;
  wf::DevArray<double> d_scratch;   // barrier / scalar reductions: one double in, one out
};

// not part of the public ABI (cg.hip): the ghost positions, for reductions over owned entries only
extern "C" int wf_updater_ghosts(const wf_updater* u, const int32_t** d_ghost_pos, int32_t* nghost);
