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

// Device memory, pinned host memory and events, recorded as they are taken and given back by reset() / the destructor: the one place
// in the library that allocates and frees them.  Every taker makes room in its list first, so nothing can throw between taking and
// recording.  It never synchronises: whoever frees while work may still be running synchronises first.
struct DeviceOwner {
  std::vector<void*> dev, host;
  std::vector<hipEvent_t> events;
  DeviceOwner() = default;
  DeviceOwner(const DeviceOwner&) = delete;
  DeviceOwner& operator=(const DeviceOwner&) = delete;
  template <class T> static size_t bytes(size_t count) { return std::max<size_t>(count, 1) * sizeof(T); }
  template <class T> T* device(size_t count) { dev.reserve(dev.size() + 1); void* p = nullptr; MVUS_HIP(hipMalloc(&p, bytes<T>(count))); dev.push_back(p); return static_cast<T*>(p); }
  template <class T> T* mapped(size_t count) { return static_cast<T*>(host_alloc(bytes<T>(count), hipHostMallocMapped)); }
  template <class T> T* pinned(size_t count) { return static_cast<T*>(host_alloc(bytes<T>(count), hipHostMallocDefault)); }
  void* host_alloc(size_t size, unsigned flags) { host.reserve(host.size() + 1); void* p = nullptr; MVUS_HIP(hipHostMalloc(&p, size, flags)); host.push_back(p); return p; }
  hipEvent_t event(unsigned flags = hipEventDefault) { events.reserve(events.size() + 1); hipEvent_t e = nullptr; MVUS_HIP(hipEventCreateWithFlags(&e, flags)); events.push_back(e); return e; }
  bool empty() const { return dev.empty() && host.empty() && events.empty(); }
  void reset() {
    for (void* p : dev) (void)hipFree(p);
    for (void* p : host) (void)hipHostFree(p);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    dev.clear(); host.clear(); events.clear();
  }
  ~DeviceOwner() { reset(); }
};

// device buffers and the stream of one stateless call, freed on every exit
struct CallBuffers {
  DeviceOwner bufs;
  hipStream_t st = nullptr;
  void open(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) throw HipError{"no usable HIP device (libmvusba has no CPU fallback)"};
    MVUS_HIP(hipSetDevice(device));
    MVUS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  }
  template <class T>
  T* get(size_t count) { return bufs.device<T>(count); }
  template <class T>
  T* put(const T* host, size_t count) { T* d = get<T>(count); if (count) MVUS_HIP(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, st)); return d; }
  ~CallBuffers() { bufs.reset(); if (st) (void)hipStreamDestroy(st); }
};

inline dim3 fit_blocks(long long cnt) { return dim3((unsigned)((cnt + 255) / 256)); }      // one thread per item, 256 a workgroup

}  // namespace mvus
