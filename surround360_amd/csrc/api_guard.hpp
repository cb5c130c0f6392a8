// api_guard.hpp — how every C-ABI entry point turns an exception into an error code and a message: one catch ladder, and the
// entry shapes as thin forms over it. Included by every file that defines entry points (api*.hip, preview.hip, jpeg.hip).
#pragma once
#include <mutex>
#include <string>

#include "../../include/s360.h"
#include "core.hpp"

namespace s360 {

// api.hip: the calling thread's last error (what s360_last_error(NULL) returns on this thread)
void set_thread_error(const std::string& m);

inline void need(bool ok, const char* what) {
  if (!ok) throw Error(S360_ERR_INVALID_ARG, what);
}

// The ladder. `fail` receives the message and stores it where the entry shape keeps it; a foreign std::exception is S360_ERR_STATE.
template <typename F, typename Fail>
int guarded(F&& f, Fail&& fail) {
  try {
    f();
    return S360_OK;
  } catch (const Error& e) {
    fail(e.what());
    return e.code;
  } catch (const std::exception& e) {
    fail(e.what());
    return S360_ERR_STATE;
  }
}
// No context (rig and file functions, and the objects that are not contexts — ISP, preview, JPEG — which are not locked): the
// message goes to the thread's error.
template <typename F>
int guard(F&& f) {
  return guarded(f, [](const char* m) { set_thread_error(m); });
}
// (Ctx is s360_ctx: a template parameter so that the files of the unlocked objects need not know the context's layout)
template <typename Ctx, typename F>
int guard(Ctx* c, F&& f) {
  // thread-safe per context: concurrent callers of one context are serialised here
  std::unique_lock<std::recursive_mutex> lk;
  if (c) lk = std::unique_lock<std::recursive_mutex>(c->mu);
  return guarded([&] { if (c) c->make_current(); f(); }, [&](const char* m) { if (c) c->err = m; set_thread_error(m); });
}
// Entry points that BLOCK on the device (a finished frame's download, waiting for uploads) give the context back while
// they wait: f receives the held lock and may unlock / relock it around the wait, so that another host thread can feed
// the next frame meanwhile (a stream's uploader beside the thread that fetches and encodes). The lock is held again before
// anything of the context is written and before the call returns.
template <typename Ctx, typename F>
int guard_l(Ctx* c, F&& f, bool needs_frame = true /* false: operator-level calls work on a context whose flags describe no frame */) {
  std::unique_lock<std::recursive_mutex> lk(c->mu);
  return guarded(
      [&] {
        c->make_current();
        if (needs_frame && !c->frame_invalid.empty()) throw Error(S360_ERR_INVALID_ARG, c->frame_invalid);
        f(lk);
        if (!lk.owns_lock()) lk.lock();
      },
      [&](const char* m) { if (!lk.owns_lock()) lk.lock(); c->err = m; set_thread_error(m); });
}
// s360_frame_* entry points: as guard, and refused when the context's flags describe no renderable frame (s360_create)
template <typename Ctx, typename F>
int frame_guard(Ctx* c, F&& f) {
  return guard(c, [&] {
    if (c && !c->frame_invalid.empty()) throw Error(S360_ERR_INVALID_ARG, c->frame_invalid);
    f();
  });
}

}  // namespace s360
