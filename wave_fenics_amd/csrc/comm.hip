// Ghost exchange behind the C ABI, part 1: the run-time binding of librccl, the RCCL
// communicator (wf_comm_*) and its file rendezvous.  The updater that exchanges
// over it is updater.hip; what the two share is comm.h.
//
// librccl is bound at run time (dlopen) so that libwavehip has no hard
// dependency on it and so that, inside a PyTorch process, the communicator is
// created in the RCCL build torch has already loaded (same SONAME librccl.so.1)
// instead of starting a second copy.
#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>

#include "comm.h"

using namespace wf;

namespace {

RcclApi* g_rccl = nullptr;

template <typename F>
bool bind(void* h, const char* name, F* fn)
{
  *fn = reinterpret_cast<F>(dlsym(h, name));
  return *fn != nullptr;
}

}  // namespace

// Loads librccl once.  Search order: $WF_RCCL_LIB, the SONAME (resolves to a copy
// already mapped into the process, e.g. PyTorch's), the ROCm install.
RcclApi* wf::rccl()
{
  if (g_rccl) return g_rccl;
  std::vector<std::string> cands;
  if (const char* e = std::getenv("WF_RCCL_LIB")) cands.push_back(e);
  cands.push_back("librccl.so.1");
  cands.push_back("librccl.so");
  cands.push_back("/opt/rocm/lib/librccl.so.1");
  std::string tried;
  for (const auto& c : cands) {
    void* h = dlopen(c.c_str(), RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
      tried += c + " (" + dlerror() + "); ";
      continue;
    }
    auto api = std::make_unique<RcclApi>();
    api->handle = h;
    api->path = c;
    bool ok = bind(h, "ncclGetVersion", &api->GetVersion) && bind(h, "ncclGetUniqueId", &api->GetUniqueId)
              && bind(h, "ncclCommInitRank", &api->CommInitRank) && bind(h, "ncclCommDestroy", &api->CommDestroy)
              && bind(h, "ncclGroupStart", &api->GroupStart) && bind(h, "ncclGroupEnd", &api->GroupEnd)
              && bind(h, "ncclSend", &api->Send) && bind(h, "ncclRecv", &api->Recv)
              && bind(h, "ncclAllReduce", &api->AllReduce) && bind(h, "ncclGetErrorString", &api->GetErrorString);
    if (!ok) {
      tried += c + " (missing symbols); ";
      dlclose(h);
      continue;
    }
    g_rccl = api.release();
    return g_rccl;
  }
  wf::set_error("RCCL not available: " + tried);
  return nullptr;
}

extern "C" {

int wf_comm_unique_id(char* id)
{
  WF_REQUIRE(id != nullptr, "wf_comm_unique_id: null output");
  RcclApi* api = rccl();
  if (!api) return WF_ERR_COMM;
  ncclUniqueId uid;
  WF_NCCL_CHECK(api, api->GetUniqueId(&uid));
  std::memcpy(id, uid.internal, WF_COMM_ID_BYTES);
  return WF_OK;
}

int wf_comm_create(const char* id, int rank, int nranks, wf_comm** out)
{
  WF_REQUIRE(id && out, "wf_comm_create: null argument");
  *out = nullptr;
  WF_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "wf_comm_create: bad rank / nranks");
  RcclApi* api = rccl();
  if (!api) return WF_ERR_COMM;
  ncclUniqueId uid;
  std::memcpy(uid.internal, id, WF_COMM_ID_BYTES);
  auto c = std::make_unique<wf_comm>();
  c->rank = rank;
  c->nranks = nranks;
  WF_NCCL_CHECK(api, api->CommInitRank(&c->comm, nranks, uid, rank));
  if (int rc = c->d_scratch.alloc(2)) return rc;
  WF_HIP_CHECK(hipMemset(c->d_scratch.data(), 0, c->d_scratch.bytes()));
  *out = c.release();
  return WF_OK;
}

// Rendezvous through a file for launchers without MPI: rank 0 writes the id to
// `path` (atomically, via rename), the others poll for it.  `path` must be unique
// per job (e.g. contain MASTER_PORT).
int wf_comm_rendezvous_file(const char* path, int rank, double timeout_s, char* id)
{
  WF_REQUIRE(path && id && rank >= 0, "wf_comm_rendezvous_file: bad argument");
  if (rank == 0) {
    int rc = wf_comm_unique_id(id);
    if (rc != WF_OK) return rc;
    const std::string tmp = std::string(path) + ".tmp";
    FILE* f = std::fopen(tmp.c_str(), "wb");
    if (!f || std::fwrite(id, 1, WF_COMM_ID_BYTES, f) != WF_COMM_ID_BYTES) {
      if (f) std::fclose(f);
      wf::set_error(std::string("wf_comm_rendezvous_file: cannot write ") + tmp);
      return WF_ERR_COMM;
    }
    std::fclose(f);
    if (std::rename(tmp.c_str(), path) != 0) {
      wf::set_error(std::string("wf_comm_rendezvous_file: cannot publish ") + path);
      return WF_ERR_COMM;
    }
    return WF_OK;
  }
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    struct stat st;
    if (stat(path, &st) == 0 && st.st_size == WF_COMM_ID_BYTES) {
      FILE* f = std::fopen(path, "rb");
      const bool ok = f && std::fread(id, 1, WF_COMM_ID_BYTES, f) == WF_COMM_ID_BYTES;
      if (f) std::fclose(f);
      if (ok) return WF_OK;
    }
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) {
      wf::set_error(std::string("wf_comm_rendezvous_file: timed out waiting for ") + path);
      return WF_ERR_COMM;
    }
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
  }
}

// rendezvous + ncclCommInitRank; rank 0 removes the file once the communicator is up
int wf_comm_create_from_file(const char* path, int rank, int nranks, double timeout_s, wf_comm** out)
{
  WF_REQUIRE(path && out, "wf_comm_create_from_file: null argument");
  *out = nullptr;
  char id[WF_COMM_ID_BYTES];
  int rc = wf_comm_rendezvous_file(path, rank, timeout_s, id);
  if (rc != WF_OK) return rc;
  rc = wf_comm_create(id, rank, nranks, out);
  if (rank == 0) (void)unlink(path);   // every rank has read it: CommInitRank returns only when all joined
  return rc;
}

int wf_comm_info(const wf_comm* comm, int* rank, int* nranks, int* rccl_version)
{
  WF_REQUIRE(comm != nullptr, "wf_comm_info: null handle");
  if (rank) *rank = comm->rank;
  if (nranks) *nranks = comm->nranks;
  if (rccl_version) {
    RcclApi* api = rccl();
    if (!api) return WF_ERR_COMM;
    WF_NCCL_CHECK(api, api->GetVersion(rccl_version));
  }
  return WF_OK;
}

int wf_comm_allreduce(wf_comm* comm, int op, int64_t count, const double* d_in, double* d_out, void* stream)
{
  WF_REQUIRE(comm && d_in && d_out && count >= 0, "wf_comm_allreduce: bad argument");
  WF_REQUIRE(op == WF_SUM || op == WF_MAX, "wf_comm_allreduce: op must be WF_SUM or WF_MAX");
  if (count == 0) return WF_OK;
  RcclApi* api = rccl();
  if (!api) return WF_ERR_COMM;
  WF_NCCL_CHECK(api, api->AllReduce(d_in, d_out, (size_t)count, kNcclFloat64, op == WF_SUM ? kNcclSum : kNcclMax,
                                    comm->comm, (hipStream_t)stream));
  return WF_OK;
}

int wf_comm_barrier(wf_comm* comm, void* stream)
{
  WF_REQUIRE(comm != nullptr, "wf_comm_barrier: null handle");
  int rc = wf_comm_allreduce(comm, WF_SUM, 1, comm->d_scratch.data(), comm->d_scratch.data() + 1, stream);
  if (rc != WF_OK) return rc;
  WF_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  return WF_OK;
}

int wf_comm_destroy(wf_comm* comm)
{
  if (!comm) return WF_OK;
  comm->d_scratch.reset();
  if (comm->comm && g_rccl) (void)g_rccl->CommDestroy(comm->comm);
  delete comm;
  return WF_OK;
}

}  // extern "C"
