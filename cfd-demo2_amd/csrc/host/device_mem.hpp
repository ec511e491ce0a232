// Device-memory plumbing of the host code: the HIP error type, the allocation
// arena, a scoped temporary buffer and the roctx range.
#pragma once
#include <hip/hip_runtime_api.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

namespace cfd2 {

struct HipError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define CFD_HIP(expr)                                                                   \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess)                                                               \
      throw ::cfd2::HipError(std::string(#expr) + ": " + hipGetErrorString(_e));        \
  } while (0)

// Device allocation arena: every buffer is freed with its owner.  Not
// copyable (a copy would free every pointer twice); swap exchanges two.
class DeviceArena {
 public:
  DeviceArena() = default;
  DeviceArena(const DeviceArena&) = delete;
  DeviceArena& operator=(const DeviceArena&) = delete;
  ~DeviceArena() { release(); }
  template <class T>
  T* alloc(size_t n) {
    void* p = nullptr;
    const size_t bytes = (n ? n : 1) * sizeof(T);
    CFD_HIP(hipMalloc(&p, bytes));
    ptrs_.push_back(p);
    bytes_ += bytes;
    return static_cast<T*>(p);
  }
  template <class T>
  T* upload(const std::vector<T>& v, hipStream_t s, size_t slack = 0) {
    // slack: zeroed elements after the data (16-byte vector reads that start
    // at any valid index, e.g. the fused prolongation's agg gathers)
    T* p = alloc<T>(v.size() + slack);
    if (slack) CFD_HIP(hipMemsetAsync(p + v.size(), 0, slack * sizeof(T), s));
    if (!v.empty()) CFD_HIP(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return p;
  }
  void swap(DeviceArena& o) {
    ptrs_.swap(o.ptrs_);
    std::swap(bytes_, o.bytes_);
  }
  void release() {
    for (void* p : ptrs_) (void)hipFree(p);
    ptrs_.clear();
    bytes_ = 0;
  }
  size_t bytes() const { return bytes_; }

 private:
  std::vector<void*> ptrs_;
  size_t bytes_ = 0;
};

// temporary device buffer (setup scratch; the arena holds what the V-cycle keeps)
template <class T>
struct DevTmp {
  T* p = nullptr;
  explicit DevTmp(size_t n) { CFD_HIP(hipMalloc(&p, (n ? n : 1) * sizeof(T))); }
  DevTmp(const DevTmp&) = delete;
  DevTmp& operator=(const DevTmp&) = delete;
  ~DevTmp() { (void)hipFree(p); }
};

// roctx range (rocprofv3 --marker-trace shows steps, Picard iterations,
// FGMRES solves and iterations, AMG setup / refresh, checkpoint I/O)
struct Range {
  explicit Range(const char* what) { roctxRangePushA(what); }
  ~Range() { roctxRangePop(); }
  Range(const Range&) = delete;
  Range& operator=(const Range&) = delete;
};

}  // namespace cfd2
