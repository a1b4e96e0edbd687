// Ghost exchange behind the C ABI, part 2: the VectorUpdater (wf_updater_*) and the overlapped apply
// (demo/gpu_scatter_mpi/VectorUpdater.hpp:21-230).
//
// The reference packs on the GPU and posts one CUDA-aware MPI_Irecv/MPI_Send per
// IndexMap neighbour.  Here the transport is RCCL over xGMI: one grouped
// ncclSend/ncclRecv per neighbour (<= 7 peers on the 2x2x2 partition = one per
// xGMI link), enqueued on a HIP stream; pack = k_gather, unpack fwd = indexed
// store, unpack rev = indexed atomic add.  Nothing synchronises with the host.
#include <memory>

#include "comm.h"

using namespace wf;

namespace {

// Move-only owner of a stream or an event, in the manner of DevArray: create() returns the WF_* code, the
// destructor destroys.  (The move constructor makes the type non-copyable.)
template <typename H, hipError_t (*Destroy)(H)>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  ~Owned() { if (h_) (void)Destroy(h_); }
  operator H() const { return h_; }

 protected:
  H h_ = nullptr;
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
  int create(int priority) { WF_HIP_CHECK(hipStreamCreateWithPriority(&h_, hipStreamNonBlocking, priority)); return WF_OK; }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
  int create() { WF_HIP_CHECK(hipEventCreateWithFlags(&h_, hipEventDisableTiming)); return WF_OK; }
};

// One side of an exchange.  Forward packs through the send lane and unpacks through the recv lane, reverse the
// other way round: the same operation with the two lanes swapped.
struct Lane {
  std::vector<int> nb;              // neighbour ranks
  std::vector<int32_t> off{0};      // segment i of d_buf goes to / comes from nb[i]  (VectorUpdater.hpp:34-46)
  DevArray<int32_t> d_idx;          // send: scatter_fwd_indices, recv: ghost positions  (VectorUpdater.hpp:49-59)
  DevArray<double> d_buf;           // (VectorUpdater.hpp:62-63)
  int32_t count = 0;

  // the host half of a lane from its descriptor fields, every entry checked; names = {side, index list, one entry}
  int fill(const char* const (&names)[3], int n, const int* neighbors, const int32_t* offsets, const int32_t* idx,
           int nranks, int ndofs)
  {
    const std::string who = "wf_updater_create: ", side = who + names[0];
    WF_REQUIRE(n == 0 || (neighbors && offsets), side + " lists missing");
    for (int i = 0; i < n; ++i) {
      WF_REQUIRE(neighbors[i] >= 0 && neighbors[i] < nranks, side + " neighbour out of range");
      WF_REQUIRE(offsets[i + 1] >= offsets[i] && offsets[0] == 0, side + " offsets not monotone");
      nb.push_back(neighbors[i]);
      off.push_back(offsets[i + 1]);
    }
    count = off.back();
    WF_REQUIRE(count == 0 || idx, who + names[1] + " missing");
    // every index the pack/unpack kernels dereference is checked on the host
    return check_index_range(idx, (size_t)count, ndofs, who + names[2] + " out of range");
  }
  int upload(const int32_t* idx)
  {
    int rc = d_idx.upload(idx, (size_t)count);
    return rc != WF_OK ? rc : d_buf.alloc((size_t)count);
  }
};
constexpr const char* kSendNames[3] = {"send", "send_indices", "send index"};
constexpr const char* kRecvNames[3] = {"recv", "ghost_positions", "ghost position"};

}  // namespace

struct wf_updater {
  wf_comm* comm = nullptr;
  bool inl = false;                 // WF_UPDATER_INLINE
  Lane send, recv;
  Stream comm_stream;               // high priority: the exchange runs here unless inl
  Event ev_packed, ev_done;         // pack -> comm_stream, comm_stream -> unpack
  // wf_op_apply_overlapped: the interior part runs on low_stream between ev_main and ev_interior
  Stream low_stream;
  Event ev_main, ev_interior;
};

namespace {

// One grouped neighbour exchange: segment i of from's buffer goes to from.nb[i], segment i of to's buffer comes
// from to.nb[i]  (VectorUpdater.hpp:113-130 / :170-188).
int exchange(wf_updater* u, const Lane& from, const Lane& to, hipStream_t s)
{
  if (from.nb.empty() && to.nb.empty()) return WF_OK;
  RcclApi* api = rccl();
  if (!api) return WF_ERR_COMM;
  WF_NCCL_CHECK(api, api->GroupStart());
  for (size_t i = 0; i < to.nb.size(); ++i) {
    const size_t cnt = (size_t)(to.off[i + 1] - to.off[i]);
    if (cnt) WF_NCCL_CHECK(api, api->Recv(to.d_buf.data() + to.off[i], cnt, kNcclFloat64, to.nb[i], u->comm->comm, s));
  }
  for (size_t i = 0; i < from.nb.size(); ++i) {
    const size_t cnt = (size_t)(from.off[i + 1] - from.off[i]);
    if (cnt) WF_NCCL_CHECK(api, api->Send(from.d_buf.data() + from.off[i], cnt, kNcclFloat64, from.nb[i], u->comm->comm, s));
  }
  WF_NCCL_CHECK(api, api->GroupEnd());
  return WF_OK;
}

// pack through `from` on `user`, exchange into `to` on the updater's stream (or inline on `user`)
int begin(wf_updater* u, const Lane& from, const Lane& to, const double* d_x, hipStream_t user, bool inl)
{
  int rc = wf_gather(from.count, from.d_idx.data(), d_x, from.d_buf.data(), user);
  if (rc != WF_OK) return rc;
  if (inl) return exchange(u, from, to, user);
  WF_HIP_CHECK(hipEventRecord(u->ev_packed, user));
  WF_HIP_CHECK(hipStreamWaitEvent(u->comm_stream, u->ev_packed, 0));
  rc = exchange(u, from, to, u->comm_stream);
  if (rc != WF_OK) return rc;
  WF_HIP_CHECK(hipEventRecord(u->ev_done, u->comm_stream));
  return WF_OK;
}

// VectorUpdater.hpp:106-131: pack the owned values the neighbours hold as ghosts, post the exchange
int fwd_begin(wf_updater* u, const double* d_x, hipStream_t s, bool inl)
{
  MarkerScope mk("update_fwd_begin");
  return begin(u, u->send, u->recv, d_x, s, inl);
}
// VectorUpdater.hpp:133-143: wait, copy into the ghost entries
int fwd_end(wf_updater* u, double* d_x, hipStream_t s, bool inl)
{
  MarkerScope mk("update_fwd_end");
  if (!inl) WF_HIP_CHECK(hipStreamWaitEvent(s, u->ev_done, 0));
  return wf_scatter_set(u->recv.count, u->recv.d_idx.data(), u->recv.d_buf.data(), d_x, s);
}
// VectorUpdater.hpp:157-189: the lanes swap roles: pack the ghost entries, send them to their owners
int rev_begin(wf_updater* u, const double* d_x, hipStream_t s, bool inl)
{
  MarkerScope mk("update_rev_begin");
  return begin(u, u->recv, u->send, d_x, s, inl);
}
// VectorUpdater.hpp:191-199: wait, accumulate into the owned entries (atomic add, scatter.cu:43)
int rev_end(wf_updater* u, double* d_x, hipStream_t s, bool inl)
{
  MarkerScope mk("update_rev_end");
  if (!inl) WF_HIP_CHECK(hipStreamWaitEvent(s, u->ev_done, 0));
  return wf_scatter_add(u->send.count, u->send.d_idx.data(), u->send.d_buf.data(), d_x, s);
}

// the halo chain of wf_op_apply_overlapped up to the reverse exchange, on the caller's stream
int chain_to_rev_begin(wf_op* op, wf_updater* u, double* d_x, double* d_y, hipStream_t s)
{
  int rc;
  if ((rc = fwd_begin(u, d_x, s, true)) != WF_OK || (rc = fwd_end(u, d_x, s, true)) != WF_OK) return rc;
  if ((rc = wf_op_apply_part(op, d_x, d_y, WF_PART_INTERFACE, s)) != WF_OK) return rc;
  return rev_begin(u, d_y, s, true);
}

// rc if it already holds an error, else the code of a HIP call
int first_error(int rc, hipError_t e, const char* what)
{
  if (rc != WF_OK || e == hipSuccess) return rc;
  set_error(std::string(what) + " failed: " + hipGetErrorString(e));
  return WF_ERR_HIP;
}

}  // namespace

extern "C" {

int wf_updater_create(wf_comm* comm, const wf_updater_desc* desc, wf_updater** out)
{
  WF_REQUIRE(desc && out, "wf_updater_create: null argument");
  *out = nullptr;
  WF_REQUIRE((desc->flags & ~WF_UPDATER_INLINE) == 0,
             "wf_updater_create: unknown bits in flags = " + std::to_string(desc->flags));
  WF_REQUIRE(desc->num_send_neighbors >= 0 && desc->num_recv_neighbors >= 0 && desc->ndofs >= 0,
             "wf_updater_create: negative size");
  WF_REQUIRE(comm || (desc->num_send_neighbors == 0 && desc->num_recv_neighbors == 0),
             "wf_updater_create: neighbours given without a communicator");
  auto u = std::make_unique<wf_updater>();
  u->comm = comm;
  u->inl = (desc->flags & WF_UPDATER_INLINE) != 0;
  const int nranks = comm ? comm->nranks : 0;
  int rc;
  // both lanes are validated before the first device call
  if ((rc = u->send.fill(kSendNames, desc->num_send_neighbors, desc->send_neighbors, desc->send_offsets, desc->send_indices,
                         nranks, desc->ndofs)) != WF_OK
      || (rc = u->recv.fill(kRecvNames, desc->num_recv_neighbors, desc->recv_neighbors, desc->recv_offsets,
                            desc->ghost_positions, nranks, desc->ndofs)) != WF_OK)
    return rc;
  if ((rc = u->send.upload(desc->send_indices)) != WF_OK || (rc = u->recv.upload(desc->ghost_positions)) != WF_OK) return rc;
  int prio_low = 0, prio_high = 0;
  WF_HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
  if ((rc = u->comm_stream.create(prio_high)) != WF_OK || (rc = u->low_stream.create(prio_low)) != WF_OK) return rc;
  for (Event* e : {&u->ev_interior, &u->ev_packed, &u->ev_done, &u->ev_main})
    if ((rc = e->create()) != WF_OK) return rc;
  *out = u.release();
  return WF_OK;
}

int wf_updater_fwd_begin(wf_updater* u, const double* d_x, void* stream)
{
  WF_REQUIRE(u && d_x, "wf_updater_fwd_begin: null argument");
  return fwd_begin(u, d_x, (hipStream_t)stream, u->inl);
}
int wf_updater_fwd_end(wf_updater* u, double* d_x, void* stream)
{
  WF_REQUIRE(u && d_x, "wf_updater_fwd_end: null argument");
  return fwd_end(u, d_x, (hipStream_t)stream, u->inl);
}
int wf_updater_rev_begin(wf_updater* u, const double* d_x, void* stream)
{
  WF_REQUIRE(u && d_x, "wf_updater_rev_begin: null argument");
  return rev_begin(u, d_x, (hipStream_t)stream, u->inl);
}
int wf_updater_rev_end(wf_updater* u, double* d_x, void* stream)
{
  WF_REQUIRE(u && d_x, "wf_updater_rev_end: null argument");
  return rev_end(u, d_x, (hipStream_t)stream, u->inl);
}
int wf_updater_fwd(wf_updater* u, double* d_x, void* stream)
{
  int rc = wf_updater_fwd_begin(u, d_x, stream);
  return rc != WF_OK ? rc : wf_updater_fwd_end(u, d_x, stream);
}
int wf_updater_rev(wf_updater* u, double* d_x, void* stream)
{
  int rc = wf_updater_rev_begin(u, d_x, stream);
  return rc != WF_OK ? rc : wf_updater_rev_end(u, d_x, stream);
}

int wf_updater_info(const wf_updater* u, int* num_send, int* num_recv, int* num_send_neighbors, int* num_recv_neighbors)
{
  WF_REQUIRE(u != nullptr, "wf_updater_info: null handle");
  if (num_send) *num_send = u->send.count;
  if (num_recv) *num_recv = u->recv.count;
  if (num_send_neighbors) *num_send_neighbors = (int)u->send.nb.size();
  if (num_recv_neighbors) *num_recv_neighbors = (int)u->recv.nb.size();
  return WF_OK;
}

int wf_updater_ghosts(const wf_updater* u, const int32_t** d_ghost_pos, int32_t* nghost)
{
  WF_REQUIRE(u && d_ghost_pos && nghost, "wf_updater_ghosts: null argument");
  *d_ghost_pos = u->recv.d_idx.data();
  *nghost = u->recv.count;
  return WF_OK;
}

int wf_updater_destroy(wf_updater* u)
{
  delete u;
  return WF_OK;
}

// y += A x on a domain-decomposed mesh with both halo directions hidden behind the
// cells that read no ghost value:
//   `stream`          : update_fwd(x) -> apply(INTERFACE) -> update_rev(y)
//   updater low_stream: apply(INTERIOR)
// and `stream` continues after both.  Needs wf_op_set_ghost_faces / wf_op_set_ghost_dofs.
//
// The halo chain (pack, RCCL, unpack, interface cells, and the same in reverse) runs on the CALLER's
// stream and the interior cells on a low-priority stream of the updater.  The chain is the longer of
// the two, so the caller's stream continues behind the reverse unpack with no cross-stream wait on
// the critical path (the interior finished earlier; waiting on a signalled event is free).  Two other
// arrangements were measured and dropped (rocprofv3 kernel trace of bench.py --periodic xyz):
//   * the mirror one (chain on a high-priority stream of the updater, interior on the caller's) paid
//     ~17 us of event latency before the caller's next kernel;
//   * a CU-masked interior stream that keeps a few CUs free for the small pack / RCCL / unpack kernels:
//     0.476 vs 0.346 ms per step, every event wait to or from the masked queue 40-60 us.
int wf_op_apply_overlapped(wf_op* op, wf_updater* u, double* d_x, double* d_y, void* stream)
{
  WF_REQUIRE(op && u && d_x && d_y, "wf_op_apply_overlapped: null argument");
  MarkerScope mk("wf_op_apply_overlapped");
  hipStream_t main = (hipStream_t)stream;
  WF_HIP_CHECK(hipEventRecord(u->ev_main, main));
  WF_HIP_CHECK(hipStreamWaitEvent(u->low_stream, u->ev_main, 0));
  int rc = wf_op_apply_part(op, d_x, d_y, WF_PART_INTERIOR, u->low_stream);
  // From here on work that writes y may be in flight on low_stream: there is one exit, and it joins
  // `stream` to ev_interior whether the steps before it succeeded or not, so that a caller who frees
  // or reuses y after an error does not race with the interior part.  The first error is returned.
  // (If the interior apply itself failed, whatever it did enqueue is still recorded and waited for.)
  rc = first_error(rc, hipEventRecord(u->ev_interior, u->low_stream), "hipEventRecord(ev_interior)");
  if (rc == WF_OK) rc = chain_to_rev_begin(op, u, d_x, d_y, main);
  // the reverse unpack adds into owned entries of y that the interior part may hold between its read and its
  // write (the owner-computes box kernel updates y with plain loads and stores): it waits for the interior
  rc = first_error(rc, hipStreamWaitEvent(main, u->ev_interior, 0), "hipStreamWaitEvent(ev_interior)");
  return rc != WF_OK ? rc : rev_end(u, d_y, main, true);
}

}  // extern "C"
