// rp_abi_host.hpp -- the host side that the libraries whose entry points take one argument block each share
// (rp_plan.hip, rp_learn.hip, rp_sac.hip, rp_droq.hip, rp_pop.hip, rp_critic.hip, rp_pop_critic.hip): the thread-local message behind <prefix>last_error, the head of an entry point
// and the launch grid's size.  Everything here has internal linkage, so each library has a message of its own.
#ifndef RP_ABI_HOST_HPP_
#define RP_ABI_HOST_HPP_

#include <hip/hip_runtime.h>

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

// The first lines of entry point `fn` (a string literal) taking `const type* a`.
#define RP_ARGS_HEAD(fn, type)                                                                      \
  if (!a) return fail(fn ": args is NULL");                                                         \
  if (a->struct_size != sizeof(type)) return fail(fn ": struct_size does not match this library's " #type)
// Returns the message of a checking routine (a std::string, empty = fine) as the entry point's error.
#define RP_ARGS_CHECK(expr)                               \
  do {                                                    \
    const std::string err_ = (expr);                      \
    if (!err_.empty()) return fail(err_);                 \
  } while (0)

unsigned blocks_for(long long total, int per) { return (unsigned)((total + per - 1) / per); }

}  // namespace

#endif  // RP_ABI_HOST_HPP_
