// rp_abi_host.hpp -- the host side that the libraries share, except the engine's (rp_engine.hip, rp_task.hip: another ABI):
//   * all fourteen: the thread-local message behind <prefix>last_error, `fail`, `HIP_OK` and the argument check;
//   * the libraries whose entry points take one argument block each (rp_plan.hip, rp_learn.hip, rp_sac.hip, rp_droq.hip,
//     rp_pop.hip, rp_critic.hip, rp_pop_critic.hip, rp_actor.hip, rp_evolve.hip): the head of an entry point and the
//     launch grid's size;
//   * the libraries with a handle (rp_render.hip, rp_audio.hip, rp_video.hip, rp_hear.hip, rp_ik.hip): the head of an
//     entry point that takes the handle, and what <prefix>create and <prefix>destroy do on the device -- a failed HIP call
//     with the entry point's name in front, the guard that destroys a half-made object, the upload of a host table and
//     the release of a list of pointers.
// Everything here has internal linkage, so each library has a message of its own.
#ifndef RP_ABI_HOST_HPP_
#define RP_ABI_HOST_HPP_

#include <hip/hip_runtime.h>

#include <initializer_list>
#include <string>

namespace {

thread_local std::string g_err;
int fail(const std::string& s) { g_err = s; return -1; }
#define HIP_OK(x)                                                                  \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess)                                                          \
      return fail(std::string(#x) + ": " + hipGetErrorString(e_));                 \
  } while (0)
// HIP_OK for <prefix>create: the message is "<entry>: <what>: <HIP's text>" (`what`: "hipMalloc", "hipMemcpy", ...).
#define HIP_OK_AS(entry, what, x)                                                              \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess)                                                                      \
      return fail(std::string(entry) + ": " + (what) + ": " + hipGetErrorString(e_));          \
  } while (0)

// The first lines of entry point `fn` (a string literal) taking `const type* a`.
#define RP_ARGS_HEAD(fn, type)                                                                      \
  if (!a) return fail(fn ": args is NULL");                                                         \
  if (a->struct_size != sizeof(type)) return fail(fn ": struct_size does not match this library's " #type)
// The first line of an entry point that takes the handle `h`; `msg` is the library's own wording.
#define RP_HANDLE_HEAD(h, msg) \
  if (!(h)) return fail(msg)
// Returns the message of a checking routine (a std::string, empty = fine) as the entry point's error.
#define RP_ARGS_CHECK(expr)                               \
  do {                                                    \
    const std::string err_ = (expr);                      \
    if (!err_.empty()) return fail(err_);                 \
  } while (0)

unsigned blocks_for(long long total, int per) { return (unsigned)((total + per - 1) / per); }

// <prefix>create's object until it is handed out: destroyed by the library's own <prefix>destroy unless released.
template <typename H>
struct CreateGuard {
  H* h;
  void (*destroy)(H*);
  ~CreateGuard() { if (h) destroy(h); }
  H* release() { H* r = h; h = nullptr; return r; }
};

// Allocates *dst and copies the `n` elements of the host array `src` into it; an empty array still gets a valid
// allocation (of one element) and no copy.  `entry`: the caller's name, for the message.
template <typename T>
int upload(const char* entry, T** dst, const T* src, size_t n) {
  HIP_OK_AS(entry, "hipMalloc", hipMalloc(dst, sizeof(T) * (n ? n : 1)));
  if (n) HIP_OK_AS(entry, "hipMemcpy", hipMemcpy(*dst, src, sizeof(T) * n, hipMemcpyHostToDevice));
  return 0;
}

// <prefix>destroy's part on the device: frees the pointers that were allocated.
void free_all(std::initializer_list<void*> ptrs) {
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
}

}  // namespace

#endif  // RP_ABI_HOST_HPP_
