// host_err.h — how a host translation unit reports a failure and brackets a profiled launch: the declarations of
// set_err / prof_begin / prof_end (defined in learner.hip), the HIPC / RC early-return macros and profiled().  Included by
// learner_internal.h and replay_internal.h, so every unit sees one definition of each.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/oprl_amd.h"

namespace oprl {
void set_err(const char* fmt, ...);
// HIP-event profiler (off by default; zero cost when off): learner.hip
void prof_begin(int kind, hipStream_t st);
void prof_end(hipStream_t st);
}  // namespace oprl
using oprl::set_err;

#define HIPC(x)                                                                        \
  do {                                                                                 \
    hipError_t _e = (x);                                                               \
    if (_e != hipSuccess) {                                                            \
      set_err("%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
      return OPRL_ERR_HIP;                                                             \
    }                                                                                  \
  } while (0)
#define RC(x)                       \
  do {                              \
    int _rc = (x);                  \
    if (_rc != OPRL_OK) return _rc; \
  } while (0)

// One launch counted and timed as profile kind `kind`: launch() returns the launcher's hipError_t
template <class F>
int profiled(int kind, hipStream_t st, F&& launch) {
  oprl::prof_begin(kind, st);
  const hipError_t e = launch();
  oprl::prof_end(st);
  HIPC(e);
  return OPRL_OK;
}
