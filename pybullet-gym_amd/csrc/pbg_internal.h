// pbg_internal.h -- what the C-ABI's translation units share (pbg_capi.hip owns the handle and the
// thread-local error message; pbg_policy.hip reaches them through these).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pbg.h"

namespace pbg {

// Set pbg_last_error()'s message and return `code`.
int capi_fail(int code, const char* msg);
// The GPU a handle lives on.
int handle_device(const pbg_handle* h);
// The global index of its env 0 (pbg_create's env_offset).
int handle_env_offset(const pbg_handle* h);

// Make `dev` the current device for a scope and put the caller's back afterwards.
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && prev >= 0 && cur != prev) (void)hipSetDevice(prev);
  }
};

}  // namespace pbg
