// The other GPUs of a renderer's process -- see device_group.h.
#include "device_group.h"

#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>
#include <thread>

#include "rccl_dl.h"
#include "renderer.h"

namespace glz {

namespace {
// One host thread per additional GPU.  One task at a time: post(), then wait().
class Worker {
 public:
  Worker() : th_([this] { loop(); }) {}
  ~Worker() { stop(); }
  void post(std::function<void()> f) {
    std::lock_guard<std::mutex> l(m_);
    task_ = std::move(f);
    has_ = true;
    done_ = false;
    cv_.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> l(m_);
    cv_.wait(l, [&] { return done_; });
  }
  void stop() {
    {
      std::lock_guard<std::mutex> l(m_);
      if (quit_) return;
      quit_ = true;
      cv_.notify_all();
    }
    th_.join();
  }

 private:
  void loop() {
    std::unique_lock<std::mutex> l(m_);
    for (;;) {
      cv_.wait(l, [&] { return has_ || quit_; });
      if (!has_) return;
      std::function<void()> f = std::move(task_);
      has_ = false;
      l.unlock();
      f();
      l.lock();
      done_ = true;
      cv_.notify_all();
    }
  }
  std::mutex m_;
  std::condition_variable cv_;
  std::function<void()> task_;
  bool has_ = false, done_ = true, quit_ = false;
  std::thread th_;   // last member: the thread starts once everything above exists
};

// The calling thread is back on the root's device when the scope ends, however it ends: for code that visits the peers' devices on the
// calling thread (the exchange, build).  Tasks posted to the peers run on their own threads and never move the caller.
struct BackOnDevice {
  int device;
  ~BackOnDevice() { (void)hipSetDevice(device); }
};

bool rccl_ok(const Rccl& nc, ncclResult_t r, const char* what, Error& err) {
  if (r == ncclSuccess) return true;
  if (err.code == 0 || err.msg.empty()) err.fail(GLZ_E_DEVICE, std::string(what) + ": " + nc.GetErrorString(r));   // the first failure is the one reported
  return false;
}
}  // namespace

// Another GPU of this process: its own instance (device + stream), a replica of the scene, a renderer for the tiles
// t % n == rank, the frame it contributes to the reduce, and the host thread that drives it.
struct DeviceGroup::Peer {
  std::unique_ptr<Instance> inst;
  std::unique_ptr<Renderer> r;
  DeviceBuffer<float4> frame;
  hipEvent_t sent = nullptr;   // peer-copy exchange: this device's tiles have left (recorded on its stream, awaited by device 0's)
  Worker worker;
  size_t n_pixels() const {   // tile slots of all its chains
    size_t n = 0;
    for (uint32_t s = 0; s < r->chains(); ++s) n += r->packed_tiles(s, false).map.n_local_pixels;
    return n;
  }
  // where its packed tiles travel from
  const float4* packed(bool result) const { return r->chains() > 1 ? frame.ptr : r->packed_tiles(0, result).data; }
  // a copy of `src` built on this device, in the shape the root's scene HAS (builder, pair leaves, flattened or two levels), not what
  // the environment of this thread would choose
  std::shared_ptr<Scene> replica_of(const Scene& src, const Instance& src_inst, Error& e) {
    inst->copy_build_options(src_inst);
    if (src.info.as_levels) inst->as_levels = (int)src.info.as_levels;
    SceneData copy = src.data;   // (current: change_scene / build have asked src.host_data() on the root's thread)
    std::shared_ptr<Scene> replica(Scene::create(inst.get(), std::move(copy), e));
    if (replica && !replica->copy_deformers(src, e)) replica.reset();
    return replica;
  }
  ~Peer() {
    worker.stop();
    if (inst) (void)hipSetDevice(inst->device);
    if (sent) (void)hipEventDestroy(sent);
    r.reset();
    frame.release();
  }
};
// What the peers' tasks write their outcome into.  The tasks hold pointers into it, so it must not go away while one of them
// runs: if the poster leaves early (an exception out of its local share of the work), the destructor waits for the workers.
struct DeviceGroup::Pending {
  std::vector<Error> errs;
  std::vector<char> ok;
  DeviceGroup* posted_on = nullptr;
  Pending() = default;
  Pending(const Pending&) = delete;
  Pending& operator=(const Pending&) = delete;
  ~Pending() {
    if (posted_on)
      for (auto& peer : posted_on->peers_) peer->worker.wait();
  }
};

DeviceGroup::DeviceGroup(Renderer& root) : root_(root) {}
DeviceGroup::~DeviceGroup() { release(); }

// f(Peer&, size_t index, Error&) -> bool on every peer's thread; f is copied into the tasks, whatever it refers to must outlive join_all()
template <class F>
void DeviceGroup::post_all(F f, Pending& p) {
  p.errs.assign(peers_.size(), Error());
  p.ok.assign(peers_.size(), 1);
  p.posted_on = this;
  for (size_t i = 0; i < peers_.size(); ++i) {
    Peer* peer = peers_[i].get();
    Error* e = &p.errs[i];
    char* ok = &p.ok[i];
    peer->worker.post([=] {
      try {
        *ok = f(*peer, i, *e) ? 1 : 0;
      } catch (const std::exception& ex) {
        e->code = GLZ_E_IO;
        e->msg = ex.what();
        *ok = 0;
      } catch (...) {   // nothing may leave a peer's thread: that would be std::terminate
        e->code = GLZ_E_IO;
        e->msg = "unknown exception on a device thread";
        *ok = 0;
      }
    });
  }
}
bool DeviceGroup::join_all(Pending& p, Error& err) {
  for (auto& peer : peers_) peer->worker.wait();
  p.posted_on = nullptr;
  for (size_t i = 0; i < p.ok.size(); ++i)
    if (!p.ok[i]) {
      err = p.errs[i];
      err.msg = "device " + std::to_string(peers_[i]->inst->device) + ": " + err.msg;
      return false;
    }
  return true;
}
// What with_peers is made of, with the whole peer for f.  The one place that answers for the calling thread's device: it is the root's
// afterwards, success or failure.
template <class F, class G>
bool DeviceGroup::on_peers(F f, G g, Error& err) {
  if (peers_.empty()) return g(err);
  BackOnDevice back{root_.instance()->device};
  Pending p;
  post_all(f, p);
  bool ok = g(err);
  Error pe;
  if (!join_all(p, pe) && ok) {
    err = pe;
    ok = false;
  }
  return ok;
}
template <class F>
bool DeviceGroup::on_peers(F f, Error& err) {
  return on_peers(f, [](Error&) { return true; }, err);
}
// f and g stay the caller's: the tasks hold a pointer to the one f
bool DeviceGroup::run(const PeerTask& f, const std::function<bool(Error&)>& g, Error& err) {
  const PeerTask* task = &f;
  return on_peers([=](Peer& p, size_t, Error& e) { return (*task)(*p.r, e); }, [&](Error& e) { return g(e); }, err);
}
Renderer& DeviceGroup::peer(size_t i) const { return *peers_[i]->r; }

void DeviceGroup::release() {
  if (!comms_.empty()) {
    std::string why;
    if (const Rccl* nc = Rccl::get(why))
      for (void* c : comms_)
        if (c) (void)nc->CommDestroy(static_cast<ncclComm_t>(c));
    comms_.clear();
  }
  peers_.clear();
  loopback_ = false;
  if (root_.instance()) (void)hipSetDevice(root_.instance()->device);
}

const Scene* DeviceGroup::scene(int i) const {
  if (i < 1 || (size_t)i > peers_.size() || !peers_[(size_t)i - 1]->r) return nullptr;
  return peers_[(size_t)i - 1]->r->scene();
}

bool DeviceGroup::change_scene(const Scene& src, const Instance& src_inst, Error& err) {
  const Scene* s = &src;
  const Instance* si = &src_inst;
  return on_peers([=](Peer& p, size_t, Error& e) {
    std::shared_ptr<Scene> replica = p.replica_of(*s, *si, e);
    return replica && p.r->change_scene(replica, e);
  }, err);
}

bool DeviceGroup::change_resolution(uint32_t w, uint32_t h, Error& err) {
  const bool want_frame = !loopback_ && exchange_ == kExchangeReduce;
  return on_peers([=](Peer& p, size_t, Error& e) {
    if (!p.r->change_resolution(w, h, e)) return false;
    return !want_frame || hip_ok(p.frame.alloc((size_t)w * h), "alloc peer frame", e);
  }, err);
}

bool DeviceGroup::add_stats(glz_render_stats* out, Error& err) {
  if (peers_.empty()) return true;
  std::vector<glz_render_stats> ps(peers_.size());
  glz_render_stats* base = ps.data();
  if (!on_peers([=](Peer& p, size_t i, Error& e) { return p.r->get_stats(base + i, e); }, err)) return false;
  for (const glz_render_stats& q : ps) {
    out->samples += q.samples;
    out->trace_closest_ms = std::max(out->trace_closest_ms, q.trace_closest_ms);
    out->shade_ms = std::max(out->shade_ms, q.shade_ms);
    out->trace_shadow_ms = std::max(out->trace_shadow_ms, q.trace_shadow_ms);
    out->other_ms = std::max(out->other_ms, q.other_ms);
    out->closest_rays += q.closest_rays; out->shadow_rays += q.shadow_rays;
    out->closest_nodes += q.closest_nodes; out->closest_tris += q.closest_tris;
    out->shadow_nodes += q.shadow_nodes; out->shadow_tris += q.shadow_tris;
    out->hits += q.hits; out->fresh_paths += q.fresh_paths;
    for (int i = 0; i < 12; ++i) out->phase[i] += q.phase[i];
    out->tex_fetches += q.tex_fetches; out->tex_bytes += q.tex_bytes; out->alpha_tex_bytes += q.alpha_tex_bytes;
    out->light_samples += q.light_samples; out->sky_samples += q.sky_samples;
  }
  out->render_ms = out->trace_closest_ms + out->shade_ms + out->trace_shadow_ms + out->other_ms;
  return true;
}

bool DeviceGroup::check(const int* devices, int n, Plan& plan, Error& err) const {
  auto bad = [&](const char* m) {
    return err.fail(GLZ_E_ARG, m);
  };
  if (!devices || n < 1 || n > 64) return bad("set_devices: between 1 and 64 devices");
  if (devices[0] != root_.instance()->device) return bad("set_devices: the first device must be the renderer's own (glz_instance_device)");
  bool all_same = true, any_same = false;
  for (int i = 0; i < n; ++i) {
    if (devices[i] != devices[0]) all_same = false;
    for (int j = 0; j < i; ++j) any_same |= devices[i] == devices[j];
  }
  // GLAZE_MULTI_LOOPBACK: the list may name ONE device n times (tests on a one-GPU box).  Any value but `rccl`: the tiles meet
  // without RCCL (which cannot put two ranks on one GPU).  `rccl`: the exchange still goes through the RCCL entry points -- for
  // a stand-in library named by GLAZE_RCCL_LIBRARY (tests/fake_rccl), so that the n >= 2 group construction itself runs.
  const char* lbenv = getenv("GLAZE_MULTI_LOOPBACK");
  const bool dup_ok = n > 1 && all_same && lbenv != nullptr;
  plan.loopback = dup_ok && strcmp(lbenv, "rccl") != 0 && strcmp(lbenv, "peer") != 0;   // `peer`: the peer-copy exchange with n "devices" on one GPU
  if (any_same && !dup_ok) return bad("set_devices: a device is listed twice (GLAZE_MULTI_LOOPBACK=1 allows n copies of ONE device, for tests)");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) count = 0;
  for (int i = 0; i < n; ++i)
    if (devices[i] < 0 || devices[i] >= count) return bad("set_devices: HIP device ordinal out of range");
  plan.exchange = kExchangeGather;
  if (const char* x = getenv("GLAZE_MULTI_EXCHANGE")) {
    if (!strcmp(x, "reduce")) plan.exchange = kExchangeReduce;
    else if (!strcmp(x, "peer")) plan.exchange = kExchangePeerCopy;
    else if (strcmp(x, "gather")) return bad("GLAZE_MULTI_EXCHANGE must be `gather`, `reduce` or `peer`");
  }
  if (dup_ok && !strcmp(lbenv, "peer")) plan.exchange = kExchangePeerCopy;
  plan.devices = devices;
  plan.n = n;
  // RCCL first: without it nothing is touched (a renderer that already spans devices keeps them)
  plan.rccl = nullptr;
  if (n > 1 && !plan.loopback && plan.exchange != kExchangePeerCopy) {
    std::string why;
    plan.rccl = Rccl::get(why);
    if (!plan.rccl) return err.fail(GLZ_E_DEVICE, why);
  }
  return true;
}

bool DeviceGroup::build(const Plan& plan, Error& err) {
  const int n = plan.n;
  const int* devices = plan.devices;
  const Rccl* nc = plan.rccl;
  for (int i = 1; i < n; ++i) peers_.emplace_back(new Peer());
  loopback_ = plan.loopback;
  exchange_ = plan.exchange;
  // instance + scene replica (upload, BVH build) + renderer for the tiles t % n == i, on every peer's own thread
  const Renderer* root = &root_;
  if (!root_.scene()->host_data(err)) return false;   // the replicas are created from the host copy: its vertices as the device has them
  const Scene* src = root_.scene();
  const Instance* src_inst = src->instance ? src->instance : root_.instance();
  const uint32_t w = root_.width(), h = root_.height(), world = (uint32_t)n;
  const bool want_frame = !plan.loopback && plan.exchange == kExchangeReduce;
  const bool built = on_peers([=](Peer& p, size_t i, Error& e) {
    p.inst.reset(Instance::create(devices[i + 1], e));
    if (!p.inst) return false;
    std::shared_ptr<Scene> replica = p.replica_of(*src, *src_inst, e);
    if (!replica) return false;
    p.r.reset(Renderer::create(p.inst.get(), replica, w, h, e));
    if (!p.r) return false;
    p.r->take_settings(*root);   // (the allocate() that follows requests a new frame)
    if (!p.r->set_partition_local((uint32_t)i + 1, world, e)) return false;
    return !want_frame || hip_ok(p.frame.alloc((size_t)w * h), "alloc peer frame", e);
  }, err);
  if (!built) return false;
  BackOnDevice back{root_.instance()->device};   // peer access and ncclCommInitAll visit the other devices on this thread
  if (!plan.loopback && !nc) {
    // direct access between device 0 and every peer (without it the copies are staged through the host); "already enabled" is fine
    for (int i = 1; i < n; ++i) {
      if (devices[i] == devices[0]) continue;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, devices[0], devices[i]) == hipSuccess && can) {
        (void)hipSetDevice(devices[0]);
        (void)hipDeviceEnablePeerAccess(devices[i], 0);
        (void)hipSetDevice(devices[i]);
        (void)hipDeviceEnablePeerAccess(devices[0], 0);
      }
    }
    (void)hipGetLastError();
  }
  if (nc) {
    std::vector<ncclComm_t> comms((size_t)n, nullptr);
    const ncclResult_t r = nc->CommInitAll(comms.data(), n, devices);
    if (r != ncclSuccess) return err.fail(GLZ_E_DEVICE, std::string("ncclCommInitAll: ") + nc->GetErrorString(r));
    for (ncclComm_t c : comms) comms_.push_back(c);
  }
  return true;
}

bool DeviceGroup::bring_tiles(bool result, float4* dst, Error& err) {
  if (!hip_ok(hipStreamSynchronize(root_.instance()->stream), "exchange: local frame", err)) return false;
  BackOnDevice back{root_.instance()->device};   // the exchanges visit the peers' devices on this thread
  if (loopback_) return peers_gather(result, dst, err);
  return exchange_ == kExchangeReduce ? exchange_reduce(result, dst, err) : exchange_packed(result, dst, err);
}

// every peer scatters its tiles into a full frame and waits for it: into `shared` (loop-back: one device, the root's frame, nothing
// cleared) or, with shared == nullptr, into its own zero-padded p.frame
bool DeviceGroup::peers_gather(bool result, float4* shared, Error& err) {
  return on_peers([=](Peer& p, size_t, Error& e) {
    if (!hip_ok(hipSetDevice(p.inst->device), "hipSetDevice", e)) return false;
    if (!p.r->gather(result, shared ? shared : p.frame.ptr, e, shared == nullptr)) return false;
    return hip_ok(hipStreamSynchronize(p.inst->stream), "exchange: peer frame", e);
  }, err);
}

const Rccl* DeviceGroup::rccl(Error& err) const {
  std::string why;
  const Rccl* nc = Rccl::get(why);
  if (nc && comms_.size() == peers_.size() + 1) return nc;
  err.fail(GLZ_E_DEVICE, nc ? "RCCL communicators are missing" : why);
  return nullptr;
}

// the end of an RCCL exchange: the peers' streams first (their buffers are free again), the root's last -- everything has arrived when
// it is idle.  Without the peers (peer copy): the root's stream waited for every peer's copy before it scattered.
bool DeviceGroup::finish_exchange(bool peers_too, Error& err) {
  if (peers_too)
    for (auto& p : peers_) {
      if (!hip_ok(hipSetDevice(p->inst->device), "hipSetDevice", err)) return false;
      if (!hip_ok(hipStreamSynchronize(p->inst->stream), "exchange (peer)", err)) return false;
    }
  if (!hip_ok(hipSetDevice(root_.instance()->device), "hipSetDevice", err)) return false;
  return hip_ok(hipStreamSynchronize(root_.instance()->stream), "exchange (root)", err);
}

// The gather shape over either transport: every peer's packed tiles go to recv_stage_ on device 0, peer after peer in the order of
// the list, and are scattered from there.
bool DeviceGroup::exchange_packed(bool result, float4* dst, Error& err) {
  const int root_device = root_.instance()->device;
  hipStream_t st = root_.instance()->stream;
  if (!on_peers([=](Peer& p, size_t, Error& e) {
        if (!hip_ok(hipSetDevice(p.inst->device), "hipSetDevice", e)) return false;
        // the chains' own tile-major buffers are what travels: one chain is sent from where it lies, several are laid end
        // to end first so that every peer issues exactly ONE send (copies and send are ordered by the peer's stream)
        if (!p.r->settle(e)) return false;
        const uint32_t S = p.r->chains();
        if (S < 2) return true;
        const size_t total = p.n_pixels();
        size_t off = 0;
        if (p.frame.count < total && !hip_ok(p.frame.alloc(total), "alloc peer staging", e)) return false;
        for (uint32_t s = 0; s < S; ++s) {
          const Renderer::PackedTiles c = p.r->packed_tiles(s, result);
          const size_t n = c.map.n_local_pixels;
          if (n && !hip_ok(hipMemcpyAsync(p.frame.ptr + off, c.data, sizeof(float4) * n, hipMemcpyDeviceToDevice, p.inst->stream), "pack tiles", e))
            return false;
          off += n;
        }
        return true;
      }, err))
    return false;
  const Rccl* nc = nullptr;   // null: peer copy
  if (exchange_ != kExchangePeerCopy && !(nc = rccl(err))) return false;
  size_t total = 0, off = 0;
  for (auto& p : peers_) total += p->n_pixels();
  if (recv_stage_.count < total && !hip_ok(recv_stage_.alloc(total), "alloc exchange staging", err)) return false;
  if (nc && !rccl_ok(*nc, nc->GroupStart(), "ncclGroupStart", err)) return false;
  bool ok = true;
  for (size_t i = 0; ok && i < peers_.size(); ++i) {
    Peer& p = *peers_[i];
    const size_t n = p.n_pixels();
    if (!n) continue;
    const float4* src = p.packed(result);
    if (nc) {
      ok = rccl_ok(*nc, nc->Send(src, n * 4, ncclFloat, 0, static_cast<ncclComm_t>(comms_[i + 1]), p.inst->stream), "ncclSend", err) &&
           rccl_ok(*nc, nc->Recv(recv_stage_.ptr + off, n * 4, ncclFloat, (int)i + 1, static_cast<ncclComm_t>(comms_[0]), st), "ncclRecv", err);
    } else {
      ok = hip_ok(hipSetDevice(p.inst->device), "hipSetDevice", err) && (p.sent || hip_ok(hipEventCreateWithFlags(&p.sent, hipEventDisableTiming), "event", err)) &&
           hip_ok(hipMemcpyPeerAsync(recv_stage_.ptr + off, root_device, src, p.inst->device, sizeof(float4) * n, p.inst->stream), "peer copy", err) &&
           hip_ok(hipEventRecord(p.sent, p.inst->stream), "peer copy", err);
      (void)hipSetDevice(root_device);   // for the wait that follows, not a restore
      ok = ok && hip_ok(hipStreamWaitEvent(st, p.sent, 0), "peer copy", err);
    }
    off += n;
  }
  if (nc) ok = rccl_ok(*nc, nc->GroupEnd(), "ncclGroupEnd", err) && ok;   // always closed, also after a failed call inside it
  if (!ok) return false;
  off = 0;
  for (auto& p : peers_)
    for (uint32_t s = 0; s < p->r->chains(); ++s) {
      const TileMap& m = p->r->packed_tiles(s, result).map;
      if (!hip_ok(launch_export(st, m, recv_stage_.ptr + off, dst, false), "k_export (received tiles)", err)) return false;
      off += m.n_local_pixels;
    }
  return finish_exchange(nc != nullptr, err);
}

// One ncclReduce per device over the zero-padded frames, in place on the root.
bool DeviceGroup::exchange_reduce(bool result, float4* dst, Error& err) {
  if (!peers_gather(result, nullptr, err)) return false;
  const Rccl* nc = rccl(err);
  if (!nc) return false;
  const size_t count = (size_t)root_.width() * root_.height() * 4;
  if (!rccl_ok(*nc, nc->GroupStart(), "ncclGroupStart", err)) return false;
  bool ok = rccl_ok(*nc, nc->Reduce(dst, dst, count, ncclFloat, ncclSum, 0, static_cast<ncclComm_t>(comms_[0]), root_.instance()->stream), "ncclReduce", err);   // in place on the root
  for (size_t i = 0; ok && i < peers_.size(); ++i)
    ok = rccl_ok(*nc, nc->Reduce(peers_[i]->frame.ptr, nullptr, count, ncclFloat, ncclSum, 0, static_cast<ncclComm_t>(comms_[i + 1]), peers_[i]->inst->stream), "ncclReduce", err);
  ok = rccl_ok(*nc, nc->GroupEnd(), "ncclGroupEnd", err) && ok;
  return ok && finish_exchange(true, err);
}

}  // namespace glz
