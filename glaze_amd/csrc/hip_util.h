// What every host file that calls the HIP runtime shares: the error check, and device events that are destroyed with their holder.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "parser.h"

namespace glz {

inline bool hip_ok(hipError_t e, const char* what, Error& err) {
  if (e == hipSuccess) return true;
  return err.fail(GLZ_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

// N device events for one timed run: created together, destroyed with the holder
template <int N>
struct Events {
  hipEvent_t ev[N] = {};
  Events() = default;
  Events(const Events&) = delete;
  Events& operator=(const Events&) = delete;
  bool create(Error& err, const char* what = "hipEventCreate") {
    for (auto& e : ev)
      if (!hip_ok(hipEventCreate(&e), what, err)) return false;
    return true;
  }
  ~Events() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// Two events around work on a stream
struct StreamTimer {
  Events<2> e;
  bool start(hipStream_t st, Error& err) {
    if (!e.create(err, "event")) return false;
    (void)hipEventRecord(e.ev[0], st);
    return true;
  }
  void stop(hipStream_t st) { (void)hipEventRecord(e.ev[1], st); }
  float ms() {   // waits for the stop event
    float v = 0.0f;
    (void)hipEventSynchronize(e.ev[1]);
    (void)hipEventElapsedTime(&v, e.ev[0], e.ev[1]);
    return v;
  }
};

}  // namespace glz
