// c4_host.hpp -- host-side helpers shared by the translation units of libc4a0_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/c4a0_hip.h"

#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>

namespace c4host {

// Sets the one error string behind c4_last_error_string() and returns `code` (the thread-local string and this function are
// defined in c4_session.hip, beside c4_last_error_string itself).
int fail(int code, const std::string& msg);

// Entry points run on the device of their session / stream and leave the caller's current
// device as they found it (PyTorch keeps its own notion of the current device).
class DeviceGuard {
 public:
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
    if (device >= 0 && device != prev_) { err_ = hipSetDevice(device); switched_ = err_ == hipSuccess; }
  }
  ~DeviceGuard() {
    if (switched_ && prev_ >= 0) (void)hipSetDevice(prev_);
  }
  hipError_t error() const { return err_; }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;

 private:
  int prev_ = -1;
  bool switched_ = false;
  hipError_t err_ = hipSuccess;
};

// Device a stream belongs to (-1 = the null stream: the caller's current device).
inline int stream_device(hipStream_t stream) {
  int dev = -1;
  if (stream != nullptr && hipStreamGetDevice(stream, &dev) != hipSuccess) dev = -1;
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = -1;
  return dev;
}

// More than 64 KB of dynamic LDS needs an opt-in per kernel AND per device (hipFuncSetAttribute
// acts on the current device's function object): remembered per (kernel, device).
inline hipError_t opt_in_lds(const void* kernel, int bytes, int device) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, bool> done;
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_pair(kernel, device);
  if (done.count(key)) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done[key] = true;
  return e;
}

// The one way a run-time value becomes a template argument of a launch: f is called with a value of the type that stands for
// it -- float / uint16_t for planes_dtype 0 / 1 (f32 / bf16 planes), std::true_type / std::false_type for a flag.  Whatever
// combinations do not exist as kernels are refused BEFORE the dispatch: f is instantiated for every value it may be given.
template <typename F>
void with_planes(uint32_t planes_dtype, F&& f) {
  if (planes_dtype == 0) f(float{}); else f(uint16_t{});
}
template <typename F>
void with_flag(bool flag, F&& f) {
  if (flag) f(std::true_type{}); else f(std::false_type{});
}

// one thread per element
inline dim3 grid_for(uint64_t n, int bs = 256) { return dim3((unsigned)((n + bs - 1) / bs)); }

// what the entry points of the f32 and training kernels check of their arguments, and how they report a failed launch
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool below_2_31(uint64_t rows, uint64_t ld) { return rows * ld < (1ull << 31); }
inline int launched(const char* what, hipError_t e) {
  if (e != hipSuccess) return fail(C4_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
  return C4_OK;
}

}  // namespace c4host

namespace c4f32 {

// One convolution of the f32 tower without activation (c4_f32_net.hip: f32_gemm<kConv0 | kConv, NT, 4, kEpiNone>, the summation order of
// include/c4a0_hip.h's "f32 evaluator"): first = planes [G][2][6][7] x w0 [cp][32], else x [cells][cp] x w [cp][9 cp]; y [cells][cp].
hipError_t launch_train_conv(bool first, const float* x, const float* w, const float* bias, float* y, uint32_t cells, uint32_t cp,
                             hipStream_t stream);

}  // namespace c4f32

// A HIP call inside an entry point: a failure ends the entry point with C4_ERR_HIP and "<the call>: <HIP's message>".
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess)                                                                          \
      return c4host::fail(C4_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));          \
  } while (0)

// run the rest of the entry point on the session's device; the caller's current device is restored on return
#define C4_ON_DEVICE(dev)                   \
  c4host::DeviceGuard _device_guard(dev);   \
  HIP_TRY(_device_guard.error())
// ... or on the device a stream belongs to (entry points without a session)
#define C4_ON_STREAM_DEVICE(stream) C4_ON_DEVICE(c4host::stream_device((hipStream_t)(stream)))
