// pbg_internal.h -- what the C-ABI's translation units share (pbg_capi.hip owns the handle and the
// thread-local error message; pbg_policy.hip reaches them through these).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

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

// The rule of an io struct versioned by its first field, uint32_t struct_size: a size that is one of `sizes` (the
// struct's versions, none above sizeof(T)) is accepted and `io` becomes the caller's struct_size bytes over zeros, so
// a field appended later reads as zero (its default) for an older caller; any other size is PBG_E_ARG.  `who` names the
// entry point and `type` the struct in the message.
template <class T, size_t N>
int read_versioned(const char* who, const char* type, const T* uio, const uint32_t (&sizes)[N], T* io) {
  bool known = false;
  for (const uint32_t s : sizes) known |= uio->struct_size == s;
  if (!known) {
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: io->struct_size %u is not a %s size", who, uio->struct_size, type);
    return capi_fail(PBG_E_ARG, msg);
  }
  memset(io, 0, sizeof(T));
  memcpy(io, uio, uio->struct_size);
  return PBG_OK;
}

}  // namespace pbg
