// r2l_launch.h -- how a kernel is launched, once per back end: the error slot of the C ABI, the R2L_KERNEL* macros that turn a
// workgroup program `blockfn(args, bid, nblk, lds)` into `static int r2l_launch_<x>(const ArgsT& a, int grid, void* stream)`, and
// the entries that say which back end this is and what it launched.
//
//   device (hipcc, gfx950)          a __global__ kernel + hipLaunchKernelGGL, optionally bracketed by events (r2l_timing_*)
//   R2L_EMUL + R2L_LOCKSTEP         tests/emul/r2l_lockstep_rt.h: one fiber per lane; a launch record instead of the timing
//   R2L_EMUL alone (R2L_SERIAL)     a loop over the workgroups; the tile forms of the kernels only: no R2L_KERNEL_NT_LDS, no
//                                   R2L_KERNEL_DYN_LDS
//
// It DEFINES the entries r2l_abi_version, r2l_last_error, r2l_is_device_build and r2l_timing_*, like r2l_api_impl.h, which includes
// it, defines every other entry: one translation unit per library includes them.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "r2l_common.h"

static thread_local std::string r2l_err;
static int r2l_fail(int code, const std::string& msg) {
  r2l_err = msg;
  return code;
}

// Every back end: R2L_KERNEL (R2L_NT threads, static LDS), R2L_KERNEL_OCC (... at W wavefronts per SIMD), R2L_KERNEL_V (... a
// block function with template arguments), R2L_KERNEL_NT (its own workgroup size, no LDS); all but the serial one:
// R2L_KERNEL_NT_LDS (its own workgroup size and static LDS) and R2L_KERNEL_DYN_LDS (workgroup size NT <= NT_MAX and LDS_FLOATS of
// dynamic LDS, both expressions of the launch arguments `a`).  r2l_backend_timing_*: what r2l_timing_enable / _report do here.
#ifdef R2L_LOCKSTEP
// the lock-step emulation (tests/emul/r2l_lockstep_rt.h): NT host threads per workgroup, the workgroups one after the other; a
// launch record (name -> count) stands in for the device build's event timing, so that tests can assert which kernels ran
#define R2L_IS_DEVICE_BUILD 0
static std::mutex r2l_ls_record_mutex;
static bool r2l_ls_record_on = false;
static std::map<std::string, int> r2l_ls_record;
static void r2l_ls_note(const char* name) {
  std::lock_guard<std::mutex> g(r2l_ls_record_mutex);
  if (r2l_ls_record_on) r2l_ls_record[std::string(name) + "_kernel"] += 1;
}
#define R2L_LS_KERNEL(name, ArgsT, NT_, LDSF, ...)                                                        \
  static int name(const ArgsT& a, int grid, void* stream) {                                               \
    (void)stream;                                                                                         \
    r2l_ls_note(#name);                                                                                   \
    r2l_ls::launch(#name, grid, (NT_), (size_t)(LDSF), &a,                                                \
                   [&](int b_, float* lds_) { __VA_ARGS__(a, b_, grid, lds_); });                         \
    return 0;                                                                                             \
  }
#define R2L_KERNEL_V(name, ArgsT, LDS_FLOATS, W, ...) R2L_LS_KERNEL(name, ArgsT, R2L_NT, LDS_FLOATS, __VA_ARGS__)
#define R2L_KERNEL_OCC(name, ArgsT, blockfn, LDS_FLOATS, W) R2L_LS_KERNEL(name, ArgsT, R2L_NT, LDS_FLOATS, blockfn)
#define R2L_KERNEL(name, ArgsT, blockfn, LDS_FLOATS) R2L_LS_KERNEL(name, ArgsT, R2L_NT, LDS_FLOATS, blockfn)
#define R2L_KERNEL_NT(name, ArgsT, blockfn, NT, W) R2L_LS_KERNEL(name, ArgsT, NT, 0, blockfn)
#define R2L_KERNEL_NT_LDS(name, ArgsT, NT, LDS_FLOATS, W, ...) R2L_LS_KERNEL(name, ArgsT, NT, LDS_FLOATS, __VA_ARGS__)
#define R2L_KERNEL_DYN_LDS(name, ArgsT, NT_MAX, W, NT, LDS_FLOATS, ...) R2L_LS_KERNEL(name, ArgsT, NT, LDS_FLOATS, __VA_ARGS__)
static void r2l_backend_timing_enable(bool on) {
  std::lock_guard<std::mutex> g(r2l_ls_record_mutex);
  r2l_ls_record_on = on;
  if (on) r2l_ls_record.clear();
}
static void r2l_backend_timing_report(std::string& out) {  // the launch record: "name count 0" lines (no clock in the emulation)
  std::lock_guard<std::mutex> g(r2l_ls_record_mutex);
  for (auto& kv : r2l_ls_record) out += kv.first + " " + std::to_string(kv.second) + " 0\n";
  r2l_ls_record.clear();
}
#elif defined(R2L_EMUL)
#define R2L_IS_DEVICE_BUILD 0
#define R2L_KERNEL_V(name, ArgsT, LDS_FLOATS, W, ...)                        \
  static int name(const ArgsT& a, int grid, void* stream) {                  \
    (void)stream;                                                            \
    std::vector<float> buf((size_t)(LDS_FLOATS) + 8);                        \
    float* lds = (float*)(((uintptr_t)buf.data() + 15) & ~(uintptr_t)15);    \
    for (int b = 0; b < grid; ++b) __VA_ARGS__(a, b, grid, lds);             \
    return 0;                                                                \
  }
#define R2L_KERNEL(name, ArgsT, blockfn, LDS_FLOATS) R2L_KERNEL_V(name, ArgsT, LDS_FLOATS, 1, blockfn)
#define R2L_KERNEL_OCC(name, ArgsT, blockfn, LDS_FLOATS, W) R2L_KERNEL(name, ArgsT, blockfn, LDS_FLOATS)
#define R2L_KERNEL_NT(name, ArgsT, blockfn, NT, W) R2L_KERNEL(name, ArgsT, blockfn, 4)
static void r2l_backend_timing_enable(bool) {}
static void r2l_backend_timing_report(std::string&) {}
#else
#define R2L_IS_DEVICE_BUILD 1
// Optional per-kernel timing (bench.py's roofline leg): when enabled, every launch is bracketed by
// hipEvents recorded on the stream the kernel is launched on; r2l_timing_report() synchronises the
// events and returns "name count total_ms" lines.  Off by default; costs one branch per launch.
struct R2LTimedLaunch {
  const char* name;
  hipEvent_t e0, e1;
};
static std::mutex r2l_timing_mutex;
static bool r2l_timing_on = false;
static std::vector<R2LTimedLaunch> r2l_timed;
static void r2l_time_begin(const char* name, hipStream_t s, R2LTimedLaunch& t) {
  t.name = name;
  (void)hipEventCreate(&t.e0);
  (void)hipEventCreate(&t.e1);
  (void)hipEventRecord(t.e0, s);
}
static void r2l_time_end(hipStream_t s, R2LTimedLaunch& t) {
  (void)hipEventRecord(t.e1, s);
  std::lock_guard<std::mutex> g(r2l_timing_mutex);
  r2l_timed.push_back(t);
}
static void r2l_backend_timing_enable(bool on) {
  std::lock_guard<std::mutex> g(r2l_timing_mutex);
  r2l_timing_on = on;
}
static void r2l_backend_timing_report(std::string& out) {
  std::vector<R2LTimedLaunch> v;
  {
    std::lock_guard<std::mutex> g(r2l_timing_mutex);
    v.swap(r2l_timed);
  }
  std::map<std::string, std::pair<int, double>> acc;
  for (auto& t : v) {
    (void)hipEventSynchronize(t.e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, t.e0, t.e1);
    (void)hipEventDestroy(t.e0);
    (void)hipEventDestroy(t.e1);
    auto& a = acc[t.name];
    a.first += 1;
    a.second += ms;
  }
  for (auto& kv : acc)
    out += kv.first + " " + std::to_string(kv.second.first) + " " + std::to_string(kv.second.second) + "\n";
}
// the host side of every launch wrapper `static int name(const ArgsT& a, int grid, void* stream)`: NT threads per workgroup,
// LDS_BYTES of dynamic LDS
#define R2L_LAUNCH(name, NT, LDS_BYTES)                                                                     \
  {                                                                                                         \
    R2LTimedLaunch t_;                                                                                      \
    const bool timed_ = r2l_timing_on;                                                                      \
    if (timed_) r2l_time_begin(#name "_kernel", (hipStream_t)stream, t_);                                   \
    hipLaunchKernelGGL(name##_kernel, dim3(grid), dim3(NT), LDS_BYTES, (hipStream_t)stream, a);             \
    if (timed_) r2l_time_end((hipStream_t)stream, t_);                                                      \
    const hipError_t e = hipGetLastError();                                                                 \
    if (e != hipSuccess) return r2l_fail(-10, std::string(#name ": ") + hipGetErrorString(e));              \
    return 0;                                                                                               \
  }
// LDS-free kernels with their own workgroup size (independent wavefronts)
#define R2L_KERNEL_NT(name, ArgsT, blockfn, NT, WAVES_PER_SIMD)                                 \
  __global__ __launch_bounds__(NT, WAVES_PER_SIMD) void name##_kernel(const ArgsT a) {         \
    blockfn(a, (int)blockIdx.x, (int)gridDim.x, nullptr);                                      \
  }                                                                                            \
  static int name(const ArgsT& a, int grid, void* stream) R2L_LAUNCH(name, NT, 0)
// kernels with their own workgroup size AND static LDS
#define R2L_KERNEL_NT_LDS(name, ArgsT, NT, LDS_FLOATS, WAVES_PER_SIMD, ...)                    \
  __global__ __launch_bounds__(NT, WAVES_PER_SIMD) void name##_kernel(const ArgsT a) {         \
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];                             \
    __VA_ARGS__(a, (int)blockIdx.x, (int)gridDim.x, lds);                                      \
  }                                                                                            \
  static int name(const ArgsT& a, int grid, void* stream) R2L_LAUNCH(name, NT, 0)
// ... of R2L_NT threads
#define R2L_KERNEL_V(name, ArgsT, LDS_FLOATS, WAVES_PER_SIMD, ...) \
  R2L_KERNEL_NT_LDS(name, ArgsT, R2L_NT, LDS_FLOATS, WAVES_PER_SIMD, __VA_ARGS__)
#define R2L_KERNEL_OCC(name, ArgsT, blockfn, LDS_FLOATS, WAVES_PER_SIMD) \
  R2L_KERNEL_NT_LDS(name, ArgsT, R2L_NT, LDS_FLOATS, WAVES_PER_SIMD, blockfn)
#define R2L_KERNEL(name, ArgsT, blockfn, LDS_FLOATS) R2L_KERNEL_OCC(name, ArgsT, blockfn, LDS_FLOATS, 1)
// Dynamic LDS above 48 KiB has to be granted per kernel and per device (hipFuncAttributeMaxDynamicSharedMemorySize): what each
// device of this process was granted for ONE kernel -- a static of that kernel's launch wrapper
#define R2L_MAX_DEVICES 64
struct R2LLdsGrant {
  std::mutex mu;
  size_t ok[R2L_MAX_DEVICES];  // 0: nothing granted yet (the default limit holds)
};
// before a launch of `kernel` with lds_bytes of dynamic LDS: raise the current device's grant where it does not cover them
static int r2l_lds_grant(R2LLdsGrant& g, const void* kernel, const char* name, size_t lds_bytes) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lk(g.mu);
  size_t& ok = g.ok[(unsigned)dev % R2L_MAX_DEVICES];
  if (lds_bytes > (ok ? ok : (size_t)48 * 1024)) {
    const hipError_t ea = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (ea != hipSuccess) return r2l_fail(-10, std::string(name) + ": " + hipGetErrorString(ea));
    ok = lds_bytes;
  }
  return 0;
}
// kernels whose workgroup size (NT <= NT_MAX) and LDS size follow the launch arguments
#define R2L_KERNEL_DYN_LDS(name, ArgsT, NT_MAX, WAVES_PER_SIMD, NT, LDS_FLOATS, ...)           \
  __global__ __launch_bounds__(NT_MAX, WAVES_PER_SIMD) void name##_kernel(const ArgsT a) {     \
    extern __shared__ __attribute__((aligned(16))) float r2l_dyn_lds[];                        \
    __VA_ARGS__(a, (int)blockIdx.x, (int)gridDim.x, r2l_dyn_lds);                              \
  }                                                                                            \
  static int name(const ArgsT& a, int grid, void* stream) {                                    \
    const size_t lds_bytes = sizeof(float) * (LDS_FLOATS);                                     \
    static R2LLdsGrant grant_;                                                                 \
    if (int e = r2l_lds_grant(grant_, (const void*)name##_kernel, #name, lds_bytes)) return e; \
    R2L_LAUNCH(name, NT, lds_bytes)                                                            \
  }
#endif

extern "C" {

int r2l_abi_version(void) { return R2L_ABI_VERSION; }
const char* r2l_last_error(void) { return r2l_err.c_str(); }
int r2l_is_device_build(void) { return R2L_IS_DEVICE_BUILD; }

void r2l_timing_enable(int on) { r2l_backend_timing_enable(on != 0); }

int r2l_timing_report(char* buf, size_t n) {
  std::string out;
  r2l_backend_timing_report(out);
  if (!buf || n == 0) return (int)out.size();
  const size_t m = out.size() < n - 1 ? out.size() : n - 1;
  memcpy(buf, out.data(), m);
  buf[m] = 0;
  return (int)m;
}

}  // extern "C"
