// What abi.cpp and abi_debug.cpp share: the structs behind the opaque handles of include/glaze_abi.h, the calling thread's error
// state, and the guards of an entry point.
#pragma once
#include <exception>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "glaze_abi.h"
#include "parser.h"
#include "renderer.h"
#include "scene.h"

struct glz_parsed {
  std::unique_ptr<glz::Parsed> p;
  std::vector<glz_texture> tex_view;
};
struct glz_instance {
  std::unique_ptr<glz::Instance> i;
};
struct glz_scene {
  // Shared with the renderer it is handed to (raytracer.rs:109-111 moves the scene into the renderer): the handle stays usable
  // for the info / debug hooks whatever the renderer does afterwards (destroy, change_scene), and the scene is freed when
  // the last of the two lets go.  `owned` = not handed to a renderer yet.
  std::shared_ptr<glz::Scene> s;
  bool owned = true;
};
struct glz_renderer {
  std::unique_ptr<glz::Renderer> r;
};

namespace glz {
namespace abi {
// record the failure for glz_last_error / glz_last_status (abi.cpp) and return its status
int fail(const Error& e);
int fail(int code, const char* msg);
}  // namespace abi
}  // namespace glz

// Guards every entry point: C++ exceptions (bad_alloc...) must not cross the C boundary.
#define GLZ_GUARD_BEGIN try {
#define GLZ_GUARD_END(ret)                                        \
  }                                                               \
  catch (const std::bad_alloc&) { fail(GLZ_E_IO, "out of host memory"); return ret; } \
  catch (const std::exception& ex) { fail(GLZ_E_ARG, ex.what()); return ret; }

#define GLZ_R(h) if (!(h)) return fail(GLZ_E_ARG, "renderer is null"); Error e
#define GLZ_RET(ok) return (ok) ? GLZ_OK : fail(e)
