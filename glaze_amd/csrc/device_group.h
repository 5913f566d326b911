// The other GPUs of a renderer's process (Renderer::set_devices): per peer an instance (device + stream), a replica of the scene, a renderer for
// the tiles t % n == rank and ONE host thread that enqueues its launches, one task at a time, while the caller's thread enqueues the root's
// (two kernels per launch and device; at 1/8 of a 1080p frame per GPU a launch lasts ~0.17 ms, so eight devices fed from one thread would be
// bound by the host).  What the devices share is the root's Renderer::Settings; the root forwards every change (forward / each).
//
// Rules every entry point keeps:
//  * nothing leaves a peer's thread as an exception; what the tasks write into outlives them even if the caller leaves early;
//  * the first error wins, the calling thread's before a peer's; a peer's message is prefixed `device N: `;
//  * after every call that visits other devices the calling thread's device is the root's, on success or failure.
//
// The exchange (bring_tiles): the tiles of the other GPUs meet the root's in `dst` (RCCL over xGMI; one communicator per device, every call
// of one exchange inside ONE ncclGroup issued from the calling thread, always closed, also after a failed call inside it).  Three shapes:
//  * gather (default): every peer chain SENDS its packed tile-major buffer (its share of the frame, 1/n of the bytes) straight to
//    device 0, which receives into a staging area and scatters with k_export.  xGMI is point to point: the n - 1 transfers use
//    n - 1 different links at the same time, each carrying 1/n of the frame (4 MB of a 1080p frame at n = 8).
//  * reduce (GLAZE_MULTI_EXCHANGE=reduce): one ncclReduce(sum, float) of the zero-padded W*H*4 frame per device, in place on the
//    root -- what SURVEY 8(e) names first; a ring moves the whole frame over every link (33 MB at 1080p).
//  * peer (GLAZE_MULTI_EXCHANGE=peer): the gather shape without RCCL -- one hipMemcpyPeerAsync per peer on that peer's stream into
//    the same staging area, an event per peer that device 0's stream waits for.  For machines whose RCCL cannot be loaded or will not
//    initialise (bench.py falls back to it and says so); never chosen silently.
// The tiles are disjoint, so all give the image of a one-GPU render bit for bit.  Loop-back mode (every "device" is this one;
// tests): RCCL cannot put two ranks on one GPU, and there is nothing to move -- the peers scatter their tiles straight into `dst`.
#pragma once
#include <functional>
#include <memory>
#include <vector>

#include "kernels.h"
#include "scene.h"

namespace glz {

class Renderer;
struct Rccl;

class DeviceGroup {
 public:
  explicit DeviceGroup(Renderer& root);
  ~DeviceGroup();
  size_t size() const { return peers_.size(); }   // the peers: devices 1 .. size() of set_devices
  bool empty() const { return peers_.empty(); }
  const Scene* scene(int i) const;                // the replica device i >= 1 renders; null when out of range
  void release();                                 // peers first, each on its own device; the calling thread ends on the root's

  // What check() made of a device list and the environment (GLAZE_MULTI_LOOPBACK, GLAZE_MULTI_EXCHANGE).  It touches nothing: a rejected
  // list, or RCCL missing where the exchange needs it, leaves the group as it was.  build() is for an empty group (after release()) and
  // n >= 2: the peers, each constructed on its own thread with the root's settings and the tiles t % n == i, then peer access or the
  // communicators.  Where it fails the caller releases the group.
  struct Plan {
    const int* devices;
    int n;
    bool loopback;
    int exchange;
    const Rccl* rccl;   // loaded by check() where the exchange goes through it, else null
  };
  bool check(const int* devices, int n, Plan& plan, Error& err) const;
  bool build(const Plan& plan, Error& err);

  // The peers do f(Renderer& peer, Error&) -> bool on their threads while the calling thread does g(Error&) -> bool; then the join.
  // Whatever f refers to must outlive the call (it does, as an argument).  Without peers this is g and nothing else.
  using PeerTask = std::function<bool(Renderer&, Error&)>;
  template <class F, class G>
  bool with_peers(F&& f, G&& g, Error& err) { return empty() ? g(err) : run(f, g, err); }
  template <class F>
  bool forward(F&& f, Error& err) { return with_peers(f, [](Error&) { return true; }, err); }
  template <class F>
  void each(F&& f) {   // f(Renderer& peer) on the calling thread, peer after peer: for setters that enqueue nothing
    for (size_t i = 0; i < size(); ++i) f(peer(i));
  }

  // the three forwarded calls that need more of a peer than its renderer
  bool change_scene(const Scene& src, const Instance& src_inst, Error& err);   // a replica of `src` per peer, in the shape `src` has
  bool change_resolution(uint32_t w, uint32_t h, Error& err);                  // ... and the zero-padded frames of the reduce shape
  bool add_stats(glz_render_stats* out, Error& err);   // the peers' into the root's: work counters add up, kernel times overlap (the slowest device is what the job waits for)

  bool bring_tiles(bool result, float4* dst, Error& err);   // the exchange (above): the peers' tiles into the root's gathered frame

 private:
  struct Peer;
  struct Pending;
  Renderer& peer(size_t i) const;
  bool run(const PeerTask& f, const std::function<bool(Error&)>& g, Error& err);
  template <class F> void post_all(F f, Pending& p);
  bool join_all(Pending& p, Error& err);
  template <class F, class G> bool on_peers(F f, G g, Error& err);
  template <class F> bool on_peers(F f, Error& err);
  bool peers_gather(bool result, float4* shared, Error& err);
  bool exchange_packed(bool result, float4* dst, Error& err);
  bool exchange_reduce(bool result, float4* dst, Error& err);
  bool finish_exchange(bool peers_too, Error& err);
  const Rccl* rccl(Error& err) const;   // the loaded library, if this group has its communicators

  Renderer& root_;
  std::vector<std::unique_ptr<Peer>> peers_;
  std::vector<void*> comms_;   // ncclComm_t per device (index 0 = the root); empty in loop-back mode and with peer copies
  bool loopback_ = false;      // all "devices" are this one device (GLAZE_MULTI_LOOPBACK=1, tests on a one-GPU box): no RCCL
  enum { kExchangeGather = 0, kExchangeReduce = 1, kExchangePeerCopy = 2 };
  int exchange_ = kExchangeGather;      // how the peers' tiles reach device 0; GLAZE_MULTI_EXCHANGE at check()
  DeviceBuffer<float4> recv_stage_;     // device 0: the packed tiles received from the peers (gather shape)
};

}  // namespace glz
