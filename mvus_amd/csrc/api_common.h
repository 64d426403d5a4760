// What the three translation units of libmvusba.so (ba_api.hip, spline_api.hip, twoview_api.hip) share: the HIP error type, the
// roctx ranges, the per-call device buffers and the error guard of the stateless entry points.  No kernels here.
#pragma once
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cstdlib>
#include <exception>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mvus_ba.h"

namespace mvus {

struct HipError { std::string msg; int code = MVUS_E_HIP; };   // code: the MVUS_E_* value the C ABI returns

#define MVUS_HIP(expr)                                                                              \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) throw ::mvus::HipError{std::string(#expr) + ": " + hipGetErrorString(e_)}; \
  } while (0)

// roctx ranges around the stages of a BA iteration (residual / linearise / solve / all-reduce) for rocprofv3 --marker-trace and the
// ROCm timeline tools: libroctx64.so is opened at run time when MVUS_ROCTX=1 (no link-time dependency, no cost otherwise)
struct RoctxApi {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  RoctxApi() {
    if (!std::getenv("MVUS_ROCTX")) return;
    void* lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib) lib = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_LOCAL);
    if (!lib) return;
    push = reinterpret_cast<int (*)(const char*)>(dlsym(lib, "roctxRangePushA"));
    pop = reinterpret_cast<int (*)()>(dlsym(lib, "roctxRangePop"));
    if (!push || !pop) { push = nullptr; pop = nullptr; }
  }
};
inline RoctxApi& roctx_api() { static RoctxApi a; return a; }
struct RoctxRange {
  bool on;
  explicit RoctxRange(const char* name) : on(roctx_api().push != nullptr) { if (on) roctx_api().push(name); }
  ~RoctxRange() { if (on) roctx_api().pop(); }
  RoctxRange(const RoctxRange&) = delete;
  RoctxRange& operator=(const RoctxRange&) = delete;
};

// what mvus_last_error(NULL) returns: ONE object for the whole library (defined in ba_api.hip), written by mvus_ba_create and by
// every entry point that takes no handle
extern thread_local std::string g_create_error;

// the stateless entry points run their body through this: nothing throws across the C ABI
template <class F>
int stateless(F&& fn) {
  try {
    return fn();
  } catch (const HipError& e) {
    g_create_error = e.msg;
    return e.code;
  } catch (const std::exception& e) {          // bad_alloc / length_error from the host-side tables
    g_create_error = e.what();
    return MVUS_E_INVALID;
  }
}

// a run-time flag as a type: fn(std::true_type{}) or fn(std::false_type{}), so that a launch whose template arguments follow
// the flag is written once: with_flag(hp.calib, [&](auto calib) { ... k<calib() ? 30 : 21> ... })
template <class F>
void with_flag(bool on, F&& fn) {
  if (on) fn(std::true_type{});
  else fn(std::false_type{});
}

// device buffers and the stream of one stateless call, freed on every exit
struct CallBuffers {
  std::vector<void*> bufs;
  hipStream_t st = nullptr;
  void open(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) throw HipError{"no usable HIP device (libmvusba has no CPU fallback)"};
    MVUS_HIP(hipSetDevice(device));
    MVUS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  }
  template <class T>
  T* get(size_t count) { void* p = nullptr; MVUS_HIP(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T))); bufs.push_back(p); return static_cast<T*>(p); }
  template <class T>
  T* put(const T* host, size_t count) { T* d = get<T>(count); if (count) MVUS_HIP(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, st)); return d; }
  ~CallBuffers() { for (void* p : bufs) (void)hipFree(p); if (st) (void)hipStreamDestroy(st); }
};

inline dim3 fit_blocks(long long cnt) { return dim3((unsigned)((cnt + 255) / 256)); }      // one thread per item, 256 a workgroup

}  // namespace mvus
